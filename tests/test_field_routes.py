"""CPU: ordered optimal routes for many start cells per map, read off the field (include/nastar_field_routes.h, ``ops.field_routes``, the
planners' ``plan_many``) -- everything that needs no GPU.

1. the definition (tests/field_routes_oracle.py): its successor is that of ``fields_grad_oracle`` and of ``fields_grad_tiled_oracle.forest``;
   on the maze fixture its route cells minus the goal are ``MazeDataset.get_opt_traj``; on dyadic costs the fp64 sum of the costs of the
   cells a route leaves, rounded once, is ``dist[start]`` bit for bit, and ``dist`` falls strictly along every route; the failures;
2. the tenth header against ``_native.FIELD_ROUTE_SIGNATURES``; the library's symbols, abi, limits and workspace size;
3. every refusal the entry point makes before any HIP call, and their order;
4. the Python refusals made without a device.
"""
import inspect
import os

import numpy as np
import pytest
import torch

import field_routes_oracle as RO
import fields_grad_oracle as GO
import fields_grad_tiled_oracle as GT
import fields_oracle as FO
import heuristic_oracle as HO
from test_fields import ROOT, _defines, _prototypes, random_map

f32, f64 = np.float32, np.float64
DIRECTED = 0x0EB
MASKS = [HO.MOORE8, HO.VON_NEUMANN, DIRECTED, 0x1A7]


def _dyadic(rng, H, W, goals):
    cost, passable, goal = random_map(rng, H, W, dyadic=True)
    for _ in range(goals - 1):
        goal[int(rng.integers(H)), int(rng.integers(W))] = 1      # (may land on an obstacle: a goal that cannot be entered)
    return cost, passable.astype(f32), goal


# ---- 1: the definition ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("H,W", [(1, 1), (7, 5), (20, 45)])
def test_successor_is_the_one_of_the_gradient_oracles(H, W, mask):
    rng = np.random.default_rng([H, W, mask])
    for goals in (1, 3):
        cost, passable, goal = _dyadic(rng, H, W, goals)
        ref = GO.field_grad(cost, goal, passable, np.zeros((H, W), f32), mask)
        assert ref.status == 0
        succ = RO.successors(ref.dist, goal, passable, mask)
        live = ref.live.reshape(-1)
        assert np.array_equal(succ[live], ref.succ.reshape(-1)[live])
        assert np.array_equal(succ[live], GT.forest(ref.dist, goal, passable, mask).succ[live])
        assert (succ[~np.isfinite(ref.dist).reshape(-1)] == -1).all()


def test_routes_on_the_maze_fixture_are_get_opt_traj():
    from neural_astar.utils.data import MazeDataset
    ds = MazeDataset(os.path.join(ROOT, "tests", "golden", "data_maze32.npz"), "train")
    N = len(ds)
    dist, _, st = FO.fields(ds.map_designs[:N], ds.goal_maps[:N], ds.map_designs[:N])
    assert (st == 0).all()
    np.random.seed(11)
    checked = 0
    for n in range(N):
        starts = [ds._random_start(n) for _ in range(5)]
        r = RO.routes(dist[n], ds.goal_maps[n, 0], ds.map_designs[n], starts)
        assert (r.status == 0).all()
        for s, n0 in enumerate(starts):
            start_map = np.zeros((1, 32, 32), f32)
            start_map.reshape(-1)[n0] = 1
            traj = ds.get_opt_traj(start_map, ds.goal_maps[n], ds.opt_policies[n])
            cells = r.cells[s]
            assert cells[0] == n0 and ds.goal_maps[n].reshape(-1)[cells[-1]] == 1 and len(set(cells)) == len(cells) == r.lengths[s]
            assert sorted(cells[:-1]) == np.flatnonzero(traj).tolist()
            assert r.costs[s] == len(cells) - 1                       # unit costs: the field counts the moves
            checked += 1
    assert checked == 5 * N


@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (9, 1), (5, 6), (20, 45), (32, 32)])
def test_route_cost_is_the_field_at_the_start_bit_for_bit(H, W):
    """dyadic costs k/64, k <= 256: every partial sum along a route is a multiple of 1/64 below 2^24 / 64, exact in fp32 and in fp64 -- so
    the field IS the sum, whatever the order"""
    reachable = longest = 0
    for mask in MASKS:
        for goals in (1, 2, 3):
            rng = np.random.default_rng([H, W, mask, goals])
            cost, passable, goal = _dyadic(rng, H, W, goals)
            dist, _, st = FO.field(cost, goal, passable, mask)
            assert st == 0
            r = RO.routes(dist, goal, passable, list(range(H * W)), mask)
            flat, c = dist.reshape(-1), cost.reshape(-1).astype(f64)
            assert np.array_equal(r.status == 0, np.isfinite(flat)) and (r.status[~np.isfinite(flat)] == RO.STATUS_UNSOLVABLE).all()
            assert np.array_equal(r.costs.view(np.uint32), flat.view(np.uint32))
            for n0, cells in enumerate(r.cells):
                if not cells:
                    assert r.lengths[n0] == 0 and (r.routes[n0] == -1).all()
                    continue
                assert f32(c[cells[:-1]].sum()).tobytes() == flat[n0].tobytes()
                assert (np.diff(flat[cells]) < 0).all() and goal.reshape(-1)[cells[-1]] != 0 and not goal.reshape(-1)[cells[:-1]].any()
                assert r.routes[n0, :len(cells)].tolist() == cells and (r.routes[n0, len(cells):] == -1).all()
                reachable, longest = reachable + 1, max(longest, len(cells))
    print(f"{H}x{W}: {reachable} reachable starts, longest route {longest} cells")
    assert reachable >= 12                                              # (1x1: the goal itself under 4 masks x 3 goal counts)


def test_failed_queries_a_short_row_and_a_plateau():
    rng = np.random.default_rng(5)
    cost, passable, goal = _dyadic(rng, 20, 45, 1)
    dist, _, _ = FO.field(cost, goal, passable)
    wall, far = int(np.flatnonzero(passable == 0)[0]), int(np.argmax(np.where(np.isfinite(dist), dist, -1)))
    gi = int(np.flatnonzero(goal)[0])
    r = RO.routes(dist, goal, passable, [-1, 900, wall, gi, far], cap=4)
    assert r.status.tolist() == [1, 1, 3, 0, 0] and r.lengths[:4].tolist() == [0, 0, 0, 1] and r.lengths[4] > 4
    assert np.isinf(r.costs[:3]).all() and r.costs[3] == 0 and r.costs[4] == dist.reshape(-1)[far]
    assert r.routes[3].tolist() == [gi, -1, -1, -1] and r.routes[4].tolist() == r.cells[4][-4:] and r.routes[4, 3] == gi
    assert (r.routes[:3] == -1).all()
    # a zero-cost corridor next to the goal: dist is 0 on it, nobody on it has a strictly closer neighbour
    cost, passable, goal = np.ones((5, 9), f32), np.ones((5, 9), f32), np.zeros((5, 9), f32)
    goal[2, 8] = 1
    cost[2, 4:8] = 0
    dist, _, _ = FO.field(cost, goal, passable)
    assert GO.field_grad(cost, goal, passable, cost).status == 11
    r = RO.routes(dist, goal, passable, [2 * 9 + 0, 2 * 9 + 5, 2 * 9 + 8, 0])
    assert r.status.tolist() == [11, 11, 0, 11] and r.lengths.tolist() == [0, 0, 1, 0] and r.costs.tolist() == [4, 0, 0, 4]


# ---- 2: header, binding, library ----------------------------------------------------------------------------------------------------------------------
NAMES = ["nastar_field_routes", "nastar_field_routes_abi", "nastar_field_routes_lds_cells", "nastar_field_routes_max_cells",
         "nastar_field_routes_workspace_bytes"]
ARGS = ["dist", "goal", "passable", "start_idx", "B", "S", "H", "W", "neighbor_mask", "routes_out", "route_cap", "route_len_out", "route_cost_out",
        "status_out", "workspace", "workspace_bytes", "stream"]


def test_tenth_header_and_field_route_signatures_agree():
    from neural_astar import _native
    protos = _prototypes("nastar_field_routes.h")
    assert sorted(protos) == sorted(_native.FIELD_ROUTE_SIGNATURES) == NAMES
    for name, (ret, args) in protos.items():
        assert _native.FIELD_ROUTE_SIGNATURES[name] == ret + " " + "".join(k for k, _ in args), name
    assert [n for _, n in protos["nastar_field_routes"][1]] == ARGS
    # a table of its own; nastar.h and the other tables are what they were
    for table in (_native.SIGNATURES, _native.ROUTE_SIGNATURES, _native.FIELD_SIGNATURES, _native.TILED_FIELD_SIGNATURES, _native.FIELD_GRAD_SIGNATURES,
                  _native.FIELD_GRAD_TILED_SIGNATURES):
        assert not set(_native.FIELD_ROUTE_SIGNATURES) & set(table)
    assert len(_prototypes("nastar.h")) == len(_native.SIGNATURES) == 74
    new = _defines("nastar_field_routes.h")
    assert new["NASTAR_FIELD_ROUTES_ABI"] == 1 and "NASTAR_VERSION" not in new and _defines("nastar.h")["NASTAR_VERSION"] == 800
    assert not [k for k in new if k.startswith("NASTAR_ERR_")]      # no new status code: 1, 3 and 11 are the other headers'
    assert (RO.STATUS_BAD_SHAPE, RO.STATUS_UNSOLVABLE, RO.STATUS_PLATEAU) == (_native.NASTAR_ERR_BAD_SHAPE, _native.NASTAR_ERR_UNSOLVABLE,
                                                                            _native.NASTAR_ERR_PLATEAU)


def test_library_exports_the_field_route_symbols():
    from neural_astar import _native, ops
    lib = _native.load()
    for sym in NAMES:
        assert hasattr(lib, sym), sym
    assert lib.nastar_field_routes_abi() == 1
    assert lib.nastar_field_routes_max_cells() == ops.FIELD_ROUTES_MAX_CELLS == lib.nastar_fields_tiled_max_cells() == 1179648
    lds = lib.nastar_field_routes_lds_cells()
    assert 16384 <= lds <= 160 * 1024 and lds < lib.nastar_field_routes_max_cells()
    assert len(lib.nastar_field_routes.argtypes) == 17
    assert {"field_routes", "FieldRoutes", "FIELD_ROUTES_MAX_CELLS"} <= set(ops.__all__)
    ws = lib.nastar_field_routes_workspace_bytes
    side = int(np.sqrt(lds)) + 1
    assert ws(1, 128, 128) == ws(7, 1, lds) == ws(1, side - 1, side - 1) == 0     # the table lives in LDS: no workspace
    assert ws(1, side, side) == (side * side + 15) // 16 * 16 and ws(3, 1, lds + 1) == (3 * (lds + 1) + 15) // 16 * 16
    assert ws(2048, 1024, 1024) == 1 << 31 and ws(1, 1024, 1152) == 1179648       # size_t throughout
    for refused in ((0, 512, 512), (1, 0, 512), (1, 512, -1), (1, 1024, 1153), (1, 65536, 65536), (-1, 512, 512)):
        assert ws(*refused) == 0, refused


# ---- 3: refusals, made before any HIP call --------------------------------------------------------------------------------------------------------------
def _args(**over):
    p = 0x10000  # never dereferenced: every call below is refused on its arguments
    a = dict(dist=p, goal=p, passable=p, start_idx=p, B=2, S=5, H=512, W=512, neighbor_mask=0x1EF, routes_out=p, route_cap=16, route_len_out=p,
             route_cost_out=None, status_out=p, workspace=p, workspace_bytes=1 << 20, stream=None)
    assert list(a) == ARGS
    a.update(over)
    return a


@pytest.mark.parametrize("over,rc", [
    (dict(dist=None), 5), (dict(goal=None), 5), (dict(passable=None), 5), (dict(start_idx=None), 5), (dict(route_len_out=None), 5),
    (dict(status_out=None), 5),
    (dict(B=0), 1), (dict(S=0), 1), (dict(H=0), 1), (dict(W=-1), 1), (dict(route_cap=0), 1), (dict(route_cap=-4), 1),
    (dict(neighbor_mask=0x1FF), 2), (dict(neighbor_mask=0x200), 2),
    (dict(neighbor_mask=0x010, dist=None), 2),                        # the mask is looked at first
    (dict(dist=None, B=0), 5),                                         # a NULL before the shape
    (dict(S=0, H=1024, W=1153), 1),                                    # the shape before the limit
    (dict(H=1024, W=1153), 2), (dict(H=65536, W=65536), 2),
    (dict(B=1 << 20, S=(1 << 10) + 1, H=8, W=8), 2), (dict(B=1, S=(1 << 30) + 1, H=8, W=8), 2),   # more than 2^30 queries
    (dict(H=1024, W=1153, workspace_bytes=0), 2),                      # the limit before the workspace
    (dict(workspace_bytes=0), 6), (dict(workspace_bytes=2 * 512 * 512 - 1), 6), (dict(workspace=None), 6)])
def test_field_routes_refuses_bad_arguments_without_a_device(over, rc):
    from neural_astar import _native
    lib = _native.load()
    assert lib.nastar_field_routes(*_args(**over).values()) == rc
    assert lib.nastar_field_routes(*_args(route_cost_out=0x10000, **over).values()) == rc
    if "route_cap" not in over:                                        # without rows the capacity is not looked at; everything else is
        assert lib.nastar_field_routes(*_args(routes_out=None, route_cap=0, **over).values()) == rc
    assert lib.nastar_last_error() == b""


def test_short_workspace_is_measured_against_the_exported_size():
    from neural_astar import _native
    lib = _native.load()
    need = lib.nastar_field_routes_workspace_bytes(2, 512, 512)
    assert need == 2 * 512 * 512
    assert lib.nastar_field_routes(*_args(workspace_bytes=need - 1).values()) == 6
    assert lib.nastar_last_error() == b""


# ---- 4: Python refusals without a device ------------------------------------------------------------------------------------------------------------------
def test_ops_and_planners_refuse_before_a_launch():
    from neural_astar import ops
    from neural_astar.planner import NeuralAstar, VanillaAstar
    from neural_astar.planner.differentiable_astar import DifferentiableAstar, FieldRoutesOutput
    assert ops.FieldRoutes._fields == ("routes", "route_lengths", "route_costs", "status")
    assert FieldRoutesOutput._fields == ("dists", "routes", "route_lengths", "route_costs", "status", "paths")
    m = torch.ones(2, 1, 8, 8)
    idx = torch.zeros(2, 3, dtype=torch.int64)
    maps = torch.zeros(2, 3, 8, 8)
    for starts in (idx, idx.int(), maps):
        with pytest.raises(RuntimeError, match="HIP device"):
            ops.field_routes(m, m, m, starts)
        with pytest.raises(RuntimeError, match="HIP device"):
            ops.field_routes(m, m, m, starts, max_route_len=7)
        with pytest.raises(RuntimeError, match="HIP device"):
            DifferentiableAstar().plan_many(m, starts, m, m)
        with pytest.raises(RuntimeError, match="HIP device"):
            VanillaAstar().plan_many(m, starts, m, paths=True)
    with pytest.raises(ValueError, match="share one"):
        ops.field_routes(m, torch.ones(2, 1, 8, 9), m, idx)
    with pytest.raises(ValueError, match="must be a"):
        ops.field_routes(torch.ones(8, 8), m, m, idx)
    with pytest.raises(TypeError, match="float32"):
        ops.field_routes(m.double(), m.double(), m.double(), idx)
    with pytest.raises(ValueError, match="neighbor_mask"):
        ops.field_routes(m, m, m, idx, neighbor_mask=0x1FF)
    for bad in (idx[0], idx[:, :0], idx[:1], idx.reshape(2, 3, 1), torch.zeros(2, 3, 8, 8, dtype=torch.int64)):
        with pytest.raises(ValueError, match="integer starts"):
            ops.field_routes(m, m, m, bad)
    for bad in (maps[0], maps[:, :0], maps[:1], torch.zeros(2, 3, 8, 9), torch.zeros(2, 3), torch.zeros(2, 3, 64)):
        with pytest.raises(ValueError, match="float starts"):
            ops.field_routes(m, m, m, bad)
    for bad in (idx.bool(), [[0, 1, 2]] * 2, None, np.zeros((2, 3), np.int32)):
        with pytest.raises(TypeError, match="starts"):
            ops.field_routes(m, m, m, bad)
    for bad in (0, -3, 1.5, True):
        with pytest.raises(ValueError, match="max_route_len"):
            ops.field_routes(m, m, m, idx, max_route_len=bad)
        with pytest.raises(ValueError, match="max_route_len"):
            DifferentiableAstar().plan_many(m, idx, m, m, max_route_len=bad)
        with pytest.raises(ValueError, match="max_route_len"):
            NeuralAstar(encoder_input="m", encoder_arch="CNN").plan_many(m, idx, m, max_route_len=bad)
    huge = torch.ones(1, 1, 1, 1).expand(1, 1, 1024, 1153)
    with pytest.raises(NotImplementedError, match="1179648"):
        ops.field_routes(huge, huge, huge, idx[:1])
    one = torch.ones(1, 1, 1, 1)
    with pytest.raises(NotImplementedError, match="queries"):
        ops.field_routes(one, one, one, torch.zeros(1, 1, dtype=torch.int32).expand(1, (1 << 30) + 1))
    # "m+": the cost map depends on the start -- one field cannot serve S starts
    with pytest.raises(NotImplementedError, match=r"planner\.astar\.plan_many\(cost_maps, "):
        NeuralAstar(encoder_input="m+", encoder_arch="CNN").plan_many(m, idx, m)


def test_start_maps_become_the_highest_index_cell():
    from neural_astar import ops
    maps = torch.zeros(2, 3, 4, 5)
    maps[0, 0, 1, 2] = 1
    maps[0, 1, 0, 0] = maps[0, 1, 3, 4] = 0.5                          # two cells: the highest index
    maps[1, 2, 0, 0] = -2
    got = ops._start_indices(maps, 2, 4, 5)
    assert got.dtype == torch.int32 and got.tolist() == [[7, 19, -1], [-1, -1, 0]]
    wide = torch.tensor([[-5, 3, 1 << 40], [20, 19, -(1 << 40)]])
    assert ops._start_indices(wide, 2, 4, 5).tolist() == [[-1, 3, 20], [20, 19, -1]]   # outside the map stays outside it
    i32 = torch.tensor([[1, 2]], dtype=torch.int32)
    assert ops._start_indices(i32, 1, 4, 5).data_ptr() == i32.data_ptr()


def test_plan_many_signatures():
    from neural_astar.planner import NeuralAstar, VanillaAstar
    from neural_astar.planner.differentiable_astar import DifferentiableAstar
    from neural_astar import ops
    assert list(inspect.signature(ops.field_routes).parameters) == ["dists", "goal_maps", "obstacles_maps", "starts", "neighbor_mask", "max_route_len"]
    assert list(inspect.signature(DifferentiableAstar.plan_many).parameters) == ["self", "cost_maps", "starts", "goal_maps", "obstacles_maps",
                                                                                "max_route_len", "paths"]
    for cls in (VanillaAstar, NeuralAstar):
        assert list(inspect.signature(cls.plan_many).parameters) == ["self", "map_designs", "starts", "goal_maps", "max_route_len", "paths"]
