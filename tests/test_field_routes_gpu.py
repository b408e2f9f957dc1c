"""GPU (-m gpu): ordered optimal routes for many start cells per map, read off the field (include/nastar_field_routes.h, ``ops.field_routes``,
the planners' ``plan_many``) against the numpy definition (tests/field_routes_oracle.py, pinned on the CPU by tests/test_field_routes.py).

Every comparison is EXACT: routes, lengths and status are integers, and a route's cost is the field's own bits at the start.  The fields the
kernel reads come from the definition (``fields_oracle``), from the device kernels, or are written by hand -- the chase is tested on all three.
"""
import functools
import os

import numpy as np
import pytest
import torch

import field_routes_oracle as RO
import fields_grad_oracle as GO
import fields_oracle as FO
import fields_tiled_oracle as TO
import heuristic_oracle as HO
from test_fields import ROOT

pytestmark = pytest.mark.gpu
f32 = np.float32
DIRECTED = 0x0EB  # one of the asymmetric move sets of the neighbour tests
SHAPES = [(1, 1), (1, 9), (7, 5), (20, 45), (32, 32), (64, 64)]
MASKS = [HO.MOORE8, HO.VON_NEUMANN, DIRECTED]


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).to(_dev())  # (a copy: the shared inputs are read-only)


@functools.lru_cache(maxsize=None)
def _maps(H, W, goals=1, seed=0):
    """3 seeded maps [3,H,W]: cost U(0.5, 1.5), passable (about 30 % obstacles; on a square map of 32 cells a side or more, map 2 is a maze of
    ``utils.synthetic`` with its own goal), goal: ``goals`` cells per map, the first on a passable cell; with more than one goal, one of
    map 0's lies on an obstacle when the map has one.  A map of 5x5 cells or more holds a WALLED-IN cell: passable, its eight neighbours
    obstacles, in the corner away from the first goal.  Shared between tests, never modified."""
    from neural_astar.utils import synthetic as syn
    rng = np.random.default_rng([seed, H, W, goals])
    B = 3
    passable = (rng.random((B, H, W)) > 0.3).astype(f32)
    goal = np.zeros((B, H, W), f32)
    for b in range(B):
        first = (int(rng.integers(H)), int(rng.integers(W)))
        passable[b][first] = 1
        if b == 2 and H == W and H >= 32:
            P = syn.maze_maps(1, H, seed=seed + 1)
            passable[b], first = P.map_designs[0, 0], tuple(np.argwhere(P.goal_maps[0, 0] != 0)[0])
        goal[b][first] = 1
        for _ in range(goals - 1):
            goal[b][int(rng.integers(H)), int(rng.integers(W))] = 1
        if H >= 5 and W >= 5:
            y, x = (1, 1) if first[0] > 2 or first[1] > 2 else (H - 2, W - 2)
            passable[b, y - 1:y + 2, x - 1:x + 2] = 0
            passable[b, y, x], goal[b, y, x] = 1, 0
    walls = np.argwhere(passable[0] == 0)
    if goals > 1 and len(walls):
        goal[0][tuple(walls[rng.integers(len(walls))])] = 1
    cost = (0.5 + rng.random((B, H, W))).astype(f32)
    for a in (cost, goal, passable):
        a.setflags(write=False)
    return cost, goal, passable


@functools.lru_cache(maxsize=None)
def _field(H, W, goals, mask, seed=0):
    cost, goal, passable = _maps(H, W, goals, seed)
    dist, _, st = FO.fields(cost, goal, passable, mask)
    assert (st == 0).all()
    dist.setflags(write=False)
    return dist


def _starts(dist, goal, passable, S, seed=0):
    """[3,S] int32.  S = 1: the reachable cell farthest from the goal.  Otherwise, per map and where the map has one: a goal cell, an
    obstacle, a walled-in cell (passable, unreachable), the indices -1 and H*W, then seeded cells from [-1, H*W]."""
    B, H, W = dist.shape
    rng = np.random.default_rng([seed, H, W, S])
    out = np.empty((B, S), np.int32)
    for b in range(B):
        d, g, p = (a[b].reshape(-1) for a in (dist, goal, passable))
        if S == 1:
            out[b, 0] = int(np.argmax(np.where(np.isfinite(d), d, -1)))
            continue
        kinds = [np.flatnonzero(g != 0), np.flatnonzero((p == 0) & (g == 0)), np.flatnonzero((p != 0) & ~np.isfinite(d))]
        special = [int(k[rng.integers(len(k))]) for k in kinds if len(k)] + [-1, H * W]
        out[b] = (special + rng.integers(-1, H * W + 1, S).tolist())[:S]
    return out


def _run(dist, goal, passable, starts, mask=None, cap=None):
    """``ops.field_routes`` on device copies -> numpy (routes, lengths, costs, status)"""
    from neural_astar import ops
    r = ops.field_routes(_t(dist)[:, None], _t(goal)[:, None], _t(passable)[:, None], _t(starts), neighbor_mask=mask, max_route_len=cap)
    B, S = starts.shape
    assert r.routes.dtype == r.route_lengths.dtype == r.status.dtype == torch.int32 and r.route_costs.dtype == torch.float32
    assert tuple(r.route_lengths.shape) == tuple(r.route_costs.shape) == tuple(r.status.shape) == (B, S) and tuple(r.routes.shape[:2]) == (B, S)
    assert cap is None or r.routes.shape[2] == cap
    return tuple(t.cpu().numpy() for t in r)


def _same(got, want, what=""):
    for g, w, name in zip(got, want, ("routes", "lengths", "costs", "status")):
        assert g.shape == w.shape, f"{what}: {name} has shape {g.shape}, the definition {w.shape}"
        same = g.view(np.uint32) == w.view(np.uint32) if name == "costs" else g == w
        assert same.all(), f"{what}: {name} differ in {int((~same).sum())} places, first at {tuple(np.argwhere(~same)[0])}"


# ---- against the definition ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("H,W", SHAPES)
def test_routes_are_the_definitions(H, W, mask):
    seen = set()
    for goals in (1, 3):
        cost, goal, passable = _maps(H, W, goals)
        dist = _field(H, W, goals, mask)
        for S in (1, 70):
            starts = _starts(dist, goal, passable, S)
            want = RO.batch(dist, goal, passable, starts, mask)
            _same(_run(dist, goal, passable, starts, mask), want, f"{H}x{W} {mask:#x} K={goals} S={S}")
            # rows of H*W entries: no route outgrows them, the chase stores on its way
            full = RO.batch(dist, goal, passable, starts, mask, cap=H * W)
            _same(_run(dist, goal, passable, starts, mask, cap=H * W), full, f"{H}x{W} {mask:#x} K={goals} S={S} cap=H*W")
            seen |= set(want[3].reshape(-1).tolist())
            if S == 70 and H * W >= 900:
                assert want[1].max() > 8 and (want[3] == 0).sum() > 70
    assert ({0, 1, 3} if H * W >= 35 else {0, 1}) <= seen <= {0, 1, 3}, seen


def test_the_starts_hold_every_kind():
    """what ``test_routes_are_the_definitions`` relies on: a goal cell, an obstacle, a walled-in cell, -1 and H*W are among the 70 starts"""
    H, W = 20, 45
    cost, goal, passable = _maps(H, W, 3)
    dist = _field(H, W, 3, HO.MOORE8)
    starts = _starts(dist, goal, passable, 70)
    assert (goal[0] * (1 - passable[0])).sum() == 1                     # one of map 0's goals lies on an obstacle
    for b in range(3):
        d, g, p = (a[b].reshape(-1) for a in (dist, goal, passable))
        inside = starts[b][(starts[b] >= 0) & (starts[b] < H * W)]
        assert g[inside].any() and (p[inside] == 0).any() and ((p[inside] != 0) & np.isinf(d[inside])).any()
        assert -1 in starts[b] and H * W in starts[b]
    on_wall = int(np.flatnonzero((goal[0] != 0) & (passable[0] == 0))[0])
    got = _run(dist, goal, passable, np.full((3, 1), on_wall, np.int32))
    assert got[3][0, 0] == 0 and got[1][0, 0] == 1 and got[0][0, 0, 0] == on_wall and got[2][0, 0] == 0   # a start on a goal: [n0], passable or not


@pytest.mark.parametrize("mask", [HO.MOORE8, HO.VON_NEUMANN])
def test_serpentine_corridor(mask):
    """16x16, a wall on every third row with one opening at alternating ends: the route from the bottom runs every corridor end to end"""
    cost, goal, passable, walls = TO.serpentine(16, 16)
    dist, _, _ = FO.field(cost, goal, passable, mask)
    rep = lambda a: np.repeat(a[None], 3, axis=0)  # noqa: E731
    starts = np.array([[255, 240, 144, 17, 0, 33]] * 3, np.int32)          # (33 = (2, 1) is a wall)
    want = RO.batch(rep(dist), rep(goal), rep(passable), starts, mask)
    _same(_run(rep(dist), rep(goal), rep(passable), starts, mask), want, f"serpentine {mask:#x}")
    assert want[1][0, :2].max() >= walls * 14 and want[3][0].tolist() == [0, 0, 0, 0, 0, 3] and want[1][0, 4] == 1
    print(f"serpentine {mask:#x}: route lengths {want[1][0].tolist()}")


@pytest.mark.parametrize("cap", [1, 5, 24])
def test_short_rows_keep_the_last_cells_and_the_true_length(cap):
    H, W = 32, 32
    cost, goal, passable = _maps(H, W, 1)
    dist = _field(H, W, 1, HO.MOORE8)
    starts = _starts(dist, goal, passable, 70)
    whole = RO.batch(dist, goal, passable, starts)
    want = RO.batch(dist, goal, passable, starts, cap=cap)
    assert np.array_equal(want[1], whole[1]) and (whole[1] > cap).any() and ((whole[1] > 0) & (whole[1] < cap)).any() == (cap > 1)
    got = _run(dist, goal, passable, starts, cap=cap)
    _same(got, want, f"cap {cap}")
    ok = got[3] == 0
    last = got[0][np.arange(3)[:, None], np.arange(70)[None], np.minimum(got[1], cap) - 1]
    assert (np.take_along_axis(goal.reshape(3, -1), np.where(ok, last, 0), 1)[ok] != 0).all()      # the goal is the last cell kept


def test_lengths_only_call():
    """routes_out NULL: lengths, costs and status alone -- and route_cost_out NULL beside it"""
    from neural_astar import _native
    H, W, S = 20, 45, 70
    cost, goal, passable = _maps(H, W, 3)
    dist = _field(H, W, 3, DIRECTED)
    starts = _starts(dist, goal, passable, S)
    want = RO.batch(dist, goal, passable, starts, DIRECTED)
    d, g, p, s = _t(dist), _t(goal), _t(passable), _t(starts)
    lengths = torch.full((3, S), -7, dtype=torch.int32, device=_dev())
    status = torch.full((3, S), -7, dtype=torch.int32, device=_dev())
    costs = torch.full((3, S), -7.0, device=_dev())
    lib = _native.load()
    stream = torch.cuda.current_stream(_dev()).cuda_stream
    for cost_out in (costs, None):
        rc = lib.nastar_field_routes(d.data_ptr(), g.data_ptr(), p.data_ptr(), s.data_ptr(), 3, S, H, W, DIRECTED, None, 0, lengths.data_ptr(),
                                     cost_out.data_ptr() if cost_out is not None else None, status.data_ptr(), None, 0, stream)
        assert rc == 0
        assert np.array_equal(lengths.cpu().numpy(), want[1]) and np.array_equal(status.cpu().numpy(), want[3])
        assert np.array_equal(costs.cpu().numpy().view(np.uint32), want[2].view(np.uint32))
        lengths.fill_(-7), status.fill_(-7)


def test_plateau_fails_the_queries_that_run_into_it_and_nobody_else():
    H, W = 5, 9
    cost, passable, goal = np.ones((3, H, W), f32), np.ones((3, H, W), f32), np.zeros((3, H, W), f32)
    goal[:, 2, 8] = 1
    cost[1, 2, 4:8] = 0                                                 # map 1: a zero-cost corridor in front of the goal
    dist = FO.fields(cost, goal, passable)[0]
    assert [GO.field_grad(cost[b], goal[b], passable[b], cost[b]).status for b in range(3)] == [0, 11, 0]
    starts = np.array([[18, 23, 26, 0, 44, 8, 36, -1]] * 3, np.int32)
    want = RO.batch(dist, goal, passable, starts)
    assert (want[3][[0, 2], :7] == 0).all() and set(want[3][1].tolist()) == {0, 1, 11} and (want[3][1, :2] == 11).all()
    for cap in (None, H * W, 2):
        _same(_run(dist, goal, passable, starts, cap=cap), RO.batch(dist, goal, passable, starts, cap=cap), f"plateau cap {cap}")


# ---- ties to what the tree already has -------------------------------------------------------------------------------------------------------------------
def test_on_unit_cost_maps_a_route_has_one_cell_more_than_the_field_says():
    from neural_astar import ops
    from neural_astar.utils import synthetic as syn
    P = syn.maze_maps(3, 32, seed=8)
    maps, goals = _t(P.map_designs), _t(P.goal_maps)
    fo = ops.cost_to_go(maps, goals, maps, policies=False)
    starts = torch.from_numpy(np.random.default_rng(2).integers(0, 1024, (3, 70)).astype(np.int64)).to(_dev())
    r = ops.field_routes(fo.dists, goals, maps, starts)
    at = fo.dists.reshape(3, -1).gather(1, starts)
    ok = torch.isfinite(at)
    assert ok.sum() > 70 and (~ok).any()
    assert torch.equal(r.status, torch.where(ok, 0, 3).int()) and torch.equal(r.route_costs, at)
    assert torch.equal(r.route_lengths[ok].float(), at[ok] + 1) and not r.route_lengths[~ok].any()
    assert r.routes.shape[2] == int(r.route_lengths.max())              # max_route_len=None: the longest route of the call


def test_route_without_its_goal_is_the_support_of_the_one_hot_gradient():
    from neural_astar import ops
    H, W = 20, 45
    cost, goal, passable = _maps(H, W, 3)
    for mask in (HO.MOORE8, DIRECTED):
        dist = _field(H, W, 3, mask)
        starts = _starts(dist, goal, passable, 1)
        G = np.zeros((3, H * W), f32)
        G[np.arange(3), starts[:, 0]] = 1
        d, g, p = _t(dist)[:, None], _t(goal)[:, None], _t(passable)[:, None]
        grad, st = ops.fields_backward(d, g, p, _t(G.reshape(3, 1, H, W)), neighbor_mask=mask)
        r = ops.field_routes(d, g, p, _t(starts), neighbor_mask=mask)
        assert st.tolist() == [0, 0, 0] and r.status.tolist() == [[0]] * 3 and int(r.route_lengths.min()) > 3
        for b in range(3):
            cells = r.routes[b, 0, :int(r.route_lengths[b, 0]) - 1].long()
            support = torch.nonzero(grad[b].reshape(-1)).flatten()
            assert torch.equal(cells.sort().values, support) and (grad[b].reshape(-1)[cells] == 1).all()


def test_on_the_maze_fixture_the_route_is_the_policy_rollout_plus_the_goal():
    from neural_astar import _native, ops
    with np.load(os.path.join(ROOT, "tests", "golden", "data_maze32.npz")) as z:
        maps, goals, pols, dists = (z[f"arr_{k}"][:3].astype(f32) for k in range(4))
    N, S = 3, 5
    rng = np.random.default_rng(6)
    starts = np.stack([rng.choice(np.flatnonzero((maps[n] != 0).reshape(-1) & (goals[n, 0] == 0).reshape(-1) & (dists[n, 0] > dists[n, 0].min()).reshape(-1)),
                                  S, replace=False) for n in range(N)]).astype(np.int32)
    m, g = _t(maps)[:, None], _t(goals)
    fo = ops.cost_to_go(m, g, m, policies=False)
    r = ops.field_routes(fo.dists, g, m, _t(starts), max_route_len=1024)
    assert r.status.tolist() == [[0] * S] * N
    pol, si, gi = _t(pols[:, :, 0]), _t(starts), _t(goals.reshape(N, -1).argmax(1).astype(np.int32))
    trajs = torch.empty((N, S, 32, 32), dtype=torch.float32, device=_dev())
    st = torch.empty((N * S,), dtype=torch.int32, device=_dev())
    rc = _native.load().nastar_policy_rollout(pol.data_ptr(), si.data_ptr(), gi.data_ptr(), N, S, 8, 32, 32, trajs.data_ptr(), st.data_ptr(),
                                              torch.cuda.current_stream(_dev()).cuda_stream)
    assert rc == 0 and st.tolist() == [0] * (N * S)
    cell = torch.where(r.routes < 0, 1024, r.routes).long()
    mask = torch.zeros((N, S, 1025), device=_dev()).scatter_(2, cell, 1.0)[..., :1024].reshape(N, S, 32, 32)
    assert torch.equal(mask, trajs + g) and torch.equal(mask.sum((2, 3)).int(), r.route_lengths)


# ---- the table in the workspace, and a field of the tiled kernel -------------------------------------------------------------------------------------------
def test_table_in_the_workspace():
    """an open unit-cost square map of the smallest side whose cell count exceeds nastar_field_routes_lds_cells(): the field, written by hand,
    is the Chebyshev distance to the goal; the third row from the bottom is a wall, the two rows below it cannot reach the goal"""
    from neural_astar import _native
    lds = _native.load().nastar_field_routes_lds_cells()
    n = int(np.sqrt(lds)) + 1
    assert (n - 1) ** 2 <= lds < n * n and _native.load().nastar_field_routes_workspace_bytes(2, n, n) >= 2 * n * n
    ys, xs = torch.meshgrid(torch.arange(n, device=_dev()), torch.arange(n, device=_dev()), indexing="ij")
    goal_at = [(3, n - 5), (n // 2 + 7, 11)]
    dist = torch.stack([torch.maximum((ys - gy).abs(), (xs - gx).abs()).float() for gy, gx in goal_at])
    passable = torch.ones((2, n, n), device=_dev())
    passable[:, n - 3] = 0
    dist[:, n - 3:] = float("inf")
    goal = torch.zeros((2, n, n), device=_dev())
    for b, (gy, gx) in enumerate(goal_at):
        goal[b, gy, gx] = 1
    starts = np.array([[0, n - 1, (n - 1) * n, n * n - 1, (n // 2) * n + n // 2, gy * n + gx] for gy, gx in goal_at], np.int32)
    d, g, p = (a.cpu().numpy() for a in (dist, goal, passable))
    want = RO.batch(d, g, p, starts)
    assert want[3].tolist() == [[0, 0, 3, 3, 0, 0]] * 2 and want[1].max() >= n - 12
    _same(_run(d, g, p, starts), want, f"{n}x{n}, the table in the workspace")
    _same(_run(d, g, p, starts, cap=n * n), RO.batch(d, g, p, starts, cap=n * n), f"{n}x{n}, rows of H*W entries")
    _same(_run(d, g, p, starts, cap=9), RO.batch(d, g, p, starts, cap=9), f"{n}x{n}, rows of 9 entries")


def test_field_of_the_tiled_kernel_129x128():
    from neural_astar import ops
    H, W, S = 129, 128, 70
    cost, goal, passable = _maps(H, W, 1)
    c, g, p = _t(cost)[:, None], _t(goal)[:, None], _t(passable)[:, None]
    fo, _ = ops.cost_to_go_tiled(c, g, p, policies=False)
    dist = fo.dists[:, 0].cpu().numpy()
    starts = _starts(dist, goal, passable, S)
    r = ops.field_routes(fo.dists, g, p, _t(starts))
    want = RO.batch(dist, goal, passable, starts)
    _same(tuple(t.cpu().numpy() for t in r), want, "129x128")
    assert (want[3] == 0).sum() > 70 and want[1].max() > 30


# ---- capture; the planners --------------------------------------------------------------------------------------------------------------------------------
def test_a_call_with_max_route_len_can_be_captured_and_one_without_is_refused():
    from neural_astar import ops
    H, W, S = 32, 32, 70
    cost, goal, passable = _maps(H, W, 1)
    dist = _field(H, W, 1, HO.MOORE8)
    d, g, p, s = _t(dist)[:, None], _t(goal)[:, None], _t(passable)[:, None], _t(_starts(dist, goal, passable, S))
    want = ops.field_routes(d, g, p, s, max_route_len=40)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with pytest.raises(RuntimeError, match="cannot be captured"):
            ops.field_routes(d, g, p, s)
        got = ops.field_routes(d, g, p, s, max_route_len=40)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def test_plan_many_on_the_three_planners_on_a_side_stream():
    from neural_astar.planner import NeuralAstar, VanillaAstar
    from neural_astar.planner.differentiable_astar import DifferentiableAstar
    from neural_astar.utils import synthetic as syn
    P = syn.maze_maps(3, 32, seed=4)
    rng = np.random.default_rng(9)
    starts_np = rng.integers(-1, 1025, (3, 6)).astype(np.int32)
    starts_np[0, 0], starts_np[1, 1], starts_np[2, 2] = -1, 1024, int(np.flatnonzero(P.map_designs[2, 0] == 0)[0])
    start_maps_np = np.zeros((3, 6, 1024), f32)
    inside = (starts_np >= 0) & (starts_np < 1024)
    start_maps_np[np.nonzero(inside) + (starts_np[inside],)] = 1
    cost_np = (0.5 + rng.random((3, 1, 32, 32))).astype(f32)
    torch.manual_seed(0)
    neural = NeuralAstar(encoder_input="m", encoder_arch="CNN").to(_dev()).eval()
    side = torch.cuda.Stream(_dev())
    with torch.cuda.stream(side), torch.no_grad():
        maps, goals = _t(P.map_designs) * 1.0, _t(P.goal_maps) * 1.0          # produced on the side stream
        costs, starts, start_maps = _t(cost_np) * 1.0, _t(starts_np) + 0, _t(start_maps_np).reshape(3, 6, 32, 32) * 1.0
        outs = {"vanilla": VanillaAstar().plan_many(maps, starts, goals, paths=True),
                "differentiable": DifferentiableAstar().plan_many(costs, starts, goals, maps, max_route_len=1024, paths=True),
                "start maps": DifferentiableAstar().plan_many(costs, start_maps, goals, maps, max_route_len=1024, paths=True),
                "neural": neural.plan_many(maps, starts, goals, paths=True)}
        predicted = neural.encode(maps, torch.zeros_like(goals), goals)
        side.synchronize()
    m, g = P.map_designs[:, 0], P.goal_maps[:, 0]
    ones = np.where(starts_np == 1024, -1, starts_np)                          # a start map cannot name H*W: its channel is empty, index -1
    for name, out in outs.items():
        c = {"vanilla": m, "neural": predicted[:, 0].cpu().numpy()}.get(name, cost_np[:, 0])
        dist = FO.fields(c, g, m)[0]
        assert np.array_equal(out.dists[:, 0].cpu().numpy(), dist), name
        want = RO.batch(dist, g, m, ones if name == "start maps" else starts_np, cap=1024 if "neural" != name != "vanilla" else None)
        _same(tuple(t.cpu().numpy() for t in (out.routes, out.route_lengths, out.route_costs, out.status)), want, name)
        assert out.paths.dtype == torch.int64 and tuple(out.paths.shape) == (3, 6, 32, 32) and not out.dists.requires_grad
        assert np.array_equal(out.paths.sum((2, 3)).cpu().numpy(), want[1]), name
        for b in range(3):
            for s in range(6):
                cells = want[0][b, s][want[0][b, s] >= 0]
                assert np.array_equal(np.flatnonzero(out.paths[b, s].cpu().numpy()), np.sort(cells)), (name, b, s)
    assert {0, 1, 3} <= set(outs["vanilla"].status.reshape(-1).tolist())
