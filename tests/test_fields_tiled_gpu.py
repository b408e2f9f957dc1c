"""GPU (-m gpu): the tiled cost-to-go relaxation (include/nastar_fields_tiled.h, ``ops.cost_to_go_tiled``, ``cost_to_go(..., tiled=True)``)
against the numpy definition (tests/fields_oracle.py).  Every comparison of ``dists``, ``policies`` and ``status`` is ``array_equal``: the
field is the same bits in whatever order tiles and cells are relaxed.  The shapes are written in terms of the
exported tile (th, tw): one tile, tiles one cell wide, rows and columns of tiles, widths that are no multiple of 4.
"""
import functools

import numpy as np
import pytest
import torch

import fields_oracle as FO
import fields_tiled_oracle as TO
import heuristic_oracle as HO
from test_fields_gpu import _dev, _filtered, _maps, _oracle, _same, _t

pytestmark = pytest.mark.gpu
f32 = np.float32
COSTS = ["u1", "u10", "dyadic", "zero", "binary", "inf_cell"]
MASKS = [HO.MOORE8, HO.VON_NEUMANN, 0x0EB, 0x1A7]


@functools.lru_cache(maxsize=None)
def _tile():
    from neural_astar import ops
    return ops.fields_tile()


def _shape(name):
    th, tw = _tile()
    return {"one": (th, tw), "plus1": (th + 1, tw + 1), "70x130": (70, 130), "129x128": (129, 128), "row": (1, 3 * tw + 5), "col": (3 * th + 5, 1),
            "130x259": (130, 259)}[name]


def _run(cost, goal, passable, mask=None, policies=True, **kw):
    from neural_astar import ops
    out, rounds = ops.cost_to_go_tiled(_t(cost)[:, None], _t(goal)[:, None], _t(passable)[:, None], neighbor_mask=mask, policies=policies, **kw)
    B, H, W = cost.shape
    assert out.dists.dtype == torch.float32 and tuple(out.dists.shape) == (B, 1, H, W) and not out.dists.requires_grad
    assert out.status.dtype == torch.int32 and tuple(out.status.shape) == (B,)
    if policies:
        assert out.policies.dtype == torch.float32 and tuple(out.policies.shape) == (B, 8, H, W) and not out.policies.requires_grad
    else:
        assert out.policies is None
    assert isinstance(rounds, int) and 0 <= rounds <= H * W + 1
    return out, rounds


# ---- shapes ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 7])
@pytest.mark.parametrize("name", ["one", "plus1", "70x130", "129x128", "row", "col", "130x259"])
def test_shapes(name, B):
    H, W = _shape(name)
    n = min(B, 2)                                   # 7 maps are 2 distinct ones over and over: the numpy definition runs twice
    pick = [b % n for b in range(B)]
    p_obstacle = 0.2 if min(H, W) > 1 else 0.0      # (a row or a column of cells: open, so that the field runs through every tile)
    cost, goal, passable = (a[pick] for a in _maps(n, H, W, p_obstacle=p_obstacle))
    want = tuple(a[pick] for a in _oracle(n, H, W, p_obstacle=p_obstacle))
    visits = torch.full((B,), -7, dtype=torch.int32, device=_dev())
    out, rounds = _run(cost, goal, passable, visits_out=visits)
    _same(out, want, f"{H}x{W} B={B}")
    assert (want[2] == 0).all() and rounds >= 1 and int(visits.min()) >= 1 and int(visits.max()) >= rounds
    th, tw = _tile()
    if H <= th and W <= tw:
        assert rounds == 1 and visits.tolist() == [1] * B
    if H * W >= 35:
        assert np.median(np.isfinite(want[0]).reshape(B, -1).sum(1)) > H * W // 4


@pytest.mark.parametrize("H,W", [(64, 64), (65, 65), (70, 130), (1, 197), (127, 129)])
def test_tiled_and_one_workgroup_kernels_give_identical_tensors(H, W):
    from neural_astar import ops
    c, g, p = (_t(a)[:, None] for a in _maps(3, H, W, goals=2, seed=12))
    a = ops.cost_to_go(c, g, p)
    b = ops.cost_to_go(c, g, p, tiled=True)
    assert torch.equal(a.dists, b.dists) and torch.equal(a.policies, b.policies) and torch.equal(a.status, b.status)
    none = ops.cost_to_go(c, g, p, tiled=True, policies=False)
    assert none.policies is None and torch.equal(none.dists, a.dists)


@pytest.mark.parametrize("kind", COSTS)
@pytest.mark.parametrize("name", ["plus1", "70x130"])
def test_costs(name, kind):
    H, W = _shape(name)
    want = _oracle(2, H, W, kind, seed=1)
    _same(_run(*_maps(2, H, W, kind, seed=1))[0], want, kind)
    d, pol, _ = want
    if kind == "zero":
        assert set(np.unique(d).tolist()) <= {0.0, np.inf} and (d == 0).sum() > 2 and not pol.any()
    if kind == "inf_cell":
        assert (np.isinf(d) & (_maps(2, H, W, kind, seed=1)[2] != 0)).any()


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("name", ["plus1", "70x130"])
def test_masks(name, mask):
    """0x0EB and 0x1A7 are directed move sets: the marking of neighbouring tiles must not rely on symmetry"""
    H, W = _shape(name)
    want = _oracle(2, H, W, seed=2, mask=mask, p_obstacle=0.15)
    _same(_run(*_maps(2, H, W, seed=2, p_obstacle=0.15), mask=mask)[0], want, hex(mask))
    assert np.isfinite(want[0]).reshape(2, -1).sum(1).max() > 16


# ---- goals -----------------------------------------------------------------------------------------------------------------------------------
def test_walled_in_goal_in_each_corner_of_an_interior_tile():
    """the init trap: the goal's in-tile neighbours are obstacles, so its own tile lowers nothing; the tiles around it have to start active"""
    th, tw = _tile()
    H, W = 3 * th, 3 * tw
    cost, passable, goal = np.ones((4, H, W), f32), np.ones((4, H, W), f32), np.zeros((4, H, W), f32)
    for b, (cy, cx) in enumerate([(0, 0), (0, 1), (1, 0), (1, 1)]):
        gy, gx = th + cy * (th - 1), tw + cx * (tw - 1)
        goal[b, gy, gx] = 1
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if (dy or dx) and th <= gy + dy < 2 * th and tw <= gx + dx < 2 * tw:
                    passable[b, gy + dy, gx + dx] = 0
    want = FO.fields(cost, goal, passable)
    assert all(np.isfinite(want[0][b][passable[b] != 0]).all() for b in range(4))
    _same(_run(cost, goal, passable)[0], want, "corner goals")


def test_goals_on_obstacles_several_goals_no_goal_and_pockets():
    th, tw = _tile()
    H, W = 70, 130
    cost, _, passable = (a.copy() for a in _maps(4, H, W, seed=4, p_obstacle=0.2))
    goal = np.zeros((4, H, W), f32)
    # map 0: a goal ON an obstacle in the last column of a tile (only that cell is 0; the policy around it must not see the 0), and a
    # passable goal elsewhere
    goal[0, 10, tw - 1] = 1
    passable[0, 10, tw - 1] = 0
    passable[0, 9:12, tw - 2:tw + 1:2] = 1
    goal[0, 40, 20] = passable[0, 40, 20] = 1
    # map 1: three goals in three tiles
    for y, x in ((5, 5), (5, tw + 30), (th + 3, 2 * tw - 1 if 2 * tw - 1 < W else W - 1)):
        goal[1, y, x] = passable[1, y, x] = 1
    # map 2: no goal.  map 3: a pocket of passable cells walled in across the corner where four tiles meet
    passable[3] = 1
    passable[3, th - 5:th + 5, tw - 5:tw + 5] = 0
    passable[3, th - 4:th + 4, tw - 4:tw + 4] = 1
    goal[3, 0, 0] = 1
    want = FO.fields(cost, goal, passable)
    out, _ = _run(cost, goal, passable)
    _same(out, want, "goals")
    d = want[0]
    assert want[2].tolist() == [0, 0, 3, 0] and d[0, 10, tw - 1] == 0 and (d[0, 9:12, tw - 2:tw + 1:2] > 0).all()
    assert (d[1] == 0).sum() == 3 and np.isinf(d[2]).all() and not want[1][2].any()
    assert np.isinf(d[3, th - 4:th + 4, tw - 4:tw + 4]).all() and np.isfinite(d[3, H - 1, W - 1])


# ---- bad costs -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [-1.0, np.nan, -np.inf])
def test_bad_cost_fails_its_map_alone(value):
    from neural_astar import _native, ops
    th, tw = _tile()
    H, W = 70, 130
    cost, goal, passable = (a.copy() for a in _maps(3, H, W, seed=6))
    assert np.argwhere(goal[1])[0][1] < tw                 # map 1's goal sits in the first column of tiles ...
    passable[1, 3, tw + 20] = 1
    cost[1, 3, tw + 20] = value                            # ... and its bad cell in another tile
    passable[0, 3, 3] = passable[2, 3, 3] = 0              # on an obstacle cell a negative or NaN cost is not looked at
    cost[0, 3, 3], cost[2, 3, 3] = np.nan, -2.0
    cost[2, 8, 8] = -0.0
    c, g, p = (_t(a) for a in (cost, goal, passable))
    dist = torch.full((3, H, W), -7.0, device=_dev())
    pol = torch.full((3, 8, H, W), -7.0, device=_dev())
    status = torch.full((3,), -7, dtype=torch.int32, device=_dev())
    lib = _native.load()
    nbytes = lib.nastar_cost_to_go_tiled_workspace_bytes(3, H, W)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=_dev())
    rc = lib.nastar_cost_to_go_tiled(c.data_ptr(), g.data_ptr(), p.data_ptr(), 3, H, W, HO.MOORE8, dist.data_ptr(), pol.data_ptr(), status.data_ptr(),
                                     None, ws.data_ptr(), nbytes, 0, None, torch.cuda.current_stream(_dev()).cuda_stream)
    assert rc == 0
    want = FO.fields(cost, goal, passable)
    assert want[2].tolist() == [0, 9, 0] == status.tolist()
    assert np.array_equal(dist.cpu().numpy(), want[0]) and np.array_equal(pol.cpu().numpy(), want[1])
    assert bool(torch.isinf(dist[1]).all()) and not bool(pol[1].any()) and np.isfinite(want[0][0]).sum() > 1 and np.isfinite(want[0][2]).sum() > 1
    with pytest.raises(ValueError, match=r"map\(s\) \[1\]"):
        ops.cost_to_go_tiled(c[:, None], g[:, None], p[:, None])
    with pytest.raises(ValueError, match=r"map\(s\) \[1\]"):
        ops.cost_to_go(c[:, None], g[:, None], p[:, None], tiled=True)


# ---- routes that cross tile borders dozens of times ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _serpentine(H, W):
    cost, goal, passable, walls = TO.serpentine(H, W)
    return cost[None], goal[None], passable[None], walls, FO.fields(cost[None], goal[None], passable[None])


@pytest.mark.parametrize("name", ["plus1", "70x130"])
def test_serpentine(name):
    H, W = _shape(name)
    cost, goal, passable, walls, want = _serpentine(H, W)
    out, rounds = _run(cost, goal, passable)
    _same(out, want, "serpentine")
    assert np.isfinite(want[0][passable != 0]).all() and want[0].max() > walls * (W - 2)
    print(f"serpentine {H}x{W}: {walls} walls, {rounds} rounds")
    assert rounds >= walls // 2


def test_two_rounds_are_too_few_for_a_serpentine():
    """a tile runs once per round: a route that alternates between two tiles about 20 times cannot finish in 2 rounds, whatever order the
    hardware picks.  Status 10 is reported, not raised; what was computed is an upper bound, finite only where the field is."""
    th, tw = _tile()
    cost, goal, passable, walls, want = _serpentine(th + 1, tw + 1)
    assert walls >= 12
    out, rounds = _run(cost, goal, passable, max_rounds=2)
    assert out.status.tolist() == [10] and rounds == 2
    d = out.dists[:, 0].cpu().numpy()
    assert (d >= want[0]).all() and not (np.isfinite(d) & ~np.isfinite(want[0])).any() and (d > want[0]).any()
    again, rounds = _run(cost, goal, passable, max_rounds=(th + 1) * (tw + 1))   # a budget that suffices: status 0, the field
    _same(again, want, "a sufficient budget")


# ---- the data set from raw maps ---------------------------------------------------------------------------------------------------------------
def test_from_maps_above_the_one_workgroup_limit():
    from neural_astar import ops
    from neural_astar.utils import synthetic as syn
    from neural_astar.utils.data import DeviceMazeBatches, start_thresholds
    dev = _dev()
    H, W = 129, 128
    assert H * W > ops.FIELDS_MAX_CELLS
    P = syn.random_obstacle_maps(8, H, W, 0.25, seed=21)
    d, pol, st = FO.fields(P.map_designs, P.goal_maps, P.map_designs)
    assert (st == 0).all()
    worst = np.where(np.isfinite(d), d, 0).max((1, 2), keepdims=True)
    opt_dists = np.where(np.isfinite(d), -d, -(worst + 1)).astype(f32)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    new = DeviceMazeBatches.from_maps(P.map_designs, P.goal_maps, dev, batch_size=8, generator=g, num_starts=2)
    assert (new.N, new.H, new.W, new.A, new.num_starts) == (8, H, W, 8, 2)
    assert np.array_equal(new.opt_dists.cpu().numpy(), opt_dists.reshape(8, -1)) and np.array_equal(new.opt_policies.cpu().numpy(), pol)
    assert np.array_equal(new.thresholds.cpu().numpy(), start_thresholds(opt_dists[:, None], np.array([0.55, 0.70, 0.85, 1.0])))
    assert np.array_equal(new.goal_idx.cpu().numpy(), P.goal_maps.reshape(8, -1).argmax(1))
    assert np.array_equal(new.map_designs.cpu().numpy(), P.map_designs.reshape(8, 1, H, W))
    maps, starts, goals, trajs = new.sample(torch.arange(8, device=dev), check=True)   # every roll-out on the device-made policies reaches the goal
    assert int(new.last_status.abs().sum()) == 0 and new.last_status.numel() == 16
    assert tuple(trajs.shape) == (8, 2, H, W) and bool((trajs.reshape(16, -1).sum(1) >= 1).all())


# ---- against the search kernels --------------------------------------------------------------------------------------------------------------
def test_dijkstra_mode_route_cost_is_the_tiled_field_at_the_start():
    H = W = 130
    cost, goal, passable = _maps(4, H, W, "dyadic", seed=7)
    da = _filtered(HO.MOORE8)
    field = _run(cost, goal, passable)[0].dists[:, 0].cpu().numpy()
    rng = np.random.default_rng(H + W)
    verdicts = set()
    for b in range(4):
        free = np.argwhere(passable[b] != 0)
        reach = np.argwhere(np.isfinite(field[b]) & (field[b] > 0))
        pool = reach if (b % 2 and len(reach)) else free
        s = tuple(pool[rng.integers(len(pool))])
        start = np.zeros((1, 1, H, W), f32)
        start[0, 0][s] = 1
        c, g, p = (_t(a[b:b + 1])[:, None] for a in (cost, goal, passable))
        out = da.plan_routes(c, _t(start), g, p, heuristic_maps=torch.zeros_like(c))
        unsolvable = int(da.last_status[0]) == 3
        assert unsolvable == bool(np.isinf(field[b][s])), (b, s)
        if not unsolvable:
            assert int(da.last_status[0]) == 0 and float(out.route_costs[0]) == float(field[b][s]), (b, s)
        verdicts.add(unsolvable)
    assert False in verdicts


def test_planner_methods_take_tiled():
    from neural_astar.planner import VanillaAstar
    from neural_astar.utils import synthetic as syn
    P = syn.random_obstacle_maps(2, 70, 130, 0.25, seed=3)
    va = VanillaAstar(g_ratio=1.0).to(_dev()).eval()
    _same(va.cost_to_go(_t(P.map_designs), _t(P.goal_maps), tiled=True), FO.fields(P.map_designs, P.goal_maps, P.map_designs), "VanillaAstar")
    vn = _filtered(HO.VON_NEUMANN)
    cost, goal, passable = _maps(2, 70, 130, seed=2, p_obstacle=0.15)
    got = vn.cost_to_go(_t(cost)[:, None], _t(goal)[:, None], _t(passable)[:, None], tiled=True)
    _same(got, _oracle(2, 70, 130, seed=2, mask=HO.VON_NEUMANN, p_obstacle=0.15), "von Neumann filter")


# ---- the call blocks: no capture ---------------------------------------------------------------------------------------------------------------
def test_a_capturing_stream_is_refused_before_anything_is_enqueued():
    from neural_astar import ops
    c, g, p = (_t(a)[:, None] for a in _maps(2, 70, 130))
    want, _ = ops.cost_to_go_tiled(c, g, p)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        marker = c + 1.0                                           # something the capture does hold
        with pytest.raises(RuntimeError, match="cannot be captured"):
            ops.cost_to_go_tiled(c, g, p)
        with pytest.raises(RuntimeError, match="cannot be captured"):
            ops.cost_to_go(c, g, p, tiled=True)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(marker, c + 1.0)
    again, _ = ops.cost_to_go_tiled(c, g, p)                       # and the call works as before afterwards
    assert torch.equal(again.dists, want.dists) and torch.equal(again.policies, want.policies)


# ---- stream discipline -----------------------------------------------------------------------------------------------------------------------
def test_non_default_stream_with_inputs_produced_on_it():
    from neural_astar import ops
    cost, goal, passable = _maps(2, 70, 130)
    base, g, p = _t(cost)[:, None], _t(goal)[:, None], _t(passable)[:, None]
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=_dev())
    with torch.cuda.stream(side):
        filler = torch.randn(2048, 2048, device=_dev())
        for _ in range(8):                       # work queued ahead of the inputs on the same stream
            filler = filler @ filler * 1e-3
        c = base * 2.0 - base                    # == base bit for bit, produced on `side` behind the filler
        out, _ = ops.cost_to_go_tiled(c, g, p)   # every launch, copy and wait of the call is on `side`
    side.synchronize()
    _same(out, _oracle(2, 70, 130), "side stream")
