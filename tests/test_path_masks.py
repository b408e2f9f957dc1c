"""CPU: the exact shortest path as a 0/1 mask and its blackbox gradient (include/nastar_path_masks.h, ``ops.shortest_paths``, the planners'
``shortest_paths``) -- everything that needs no GPU.

1. the definition (tests/path_masks_oracle.py): the mask is the scatter of the route oracle's cells; on dyadic costs the path's cost is the
   sum of the costs under the mask minus the goal's, exactly; a hand-built 3x3 gradient, cell by cell; the failed-map conventions; the clamp;
2. the eleventh header against ``_native.PATH_MASK_SIGNATURES``; the library's symbols, abi and limit;
3. every refusal the two entry points make before any HIP call, and their order;
4. the Python refusals made without a device.
"""
import inspect

import numpy as np
import pytest
import torch

import field_routes_oracle as RO
import fields_oracle as FO
import heuristic_oracle as HO
import path_masks_oracle as PO
from test_fields import _defines, _prototypes, random_map

f32, f64 = np.float32, np.float64
DIRECTED = 0x0EB
MASKS = [HO.MOORE8, HO.VON_NEUMANN, DIRECTED]


# ---- 1: the definition ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("H,W", [(1, 1), (1, 9), (7, 5), (20, 45)])
def test_mask_is_the_scatter_of_the_route_oracle_and_its_cost_the_sum_under_it(H, W, mask):
    """dyadic costs k/64, k <= 256: every partial sum along a route is exact in fp32 and in fp64, so the field at the start IS the sum of the
    costs of the cells the route leaves: all its cells but the goal reached"""
    rng = np.random.default_rng([H, W, mask])
    solved = 0
    for _ in range(4):
        cost, passable, goal = random_map(rng, H, W, dyadic=True)
        passable = passable.astype(f32)
        dist, _, st = FO.field(cost, goal, passable, mask)
        assert st == 0
        for n0 in [int(v) for v in rng.integers(0, H * W, 6)] + [int(np.flatnonzero(goal)[0])]:
            got = PO.path(cost, goal, passable, n0, mask)
            r = RO.routes(dist, goal, passable, [n0], mask)
            assert got.status == r.status[0]
            want = np.zeros(H * W, f32)
            want[r.cells[0]] = 1
            assert np.array_equal(got.mask.reshape(-1), want) and got.cells == r.cells[0]
            if got.status:
                assert not got.mask.any() and np.isposinf(got.cost)
                continue
            assert got.cost.tobytes() == dist.reshape(-1)[n0].tobytes() == r.costs[0].tobytes()
            assert got.mask.reshape(-1)[n0] == 1 and got.mask.sum() == len(got.cells) == r.lengths[0]
            reached = got.cells[-1]
            assert goal.reshape(-1)[reached] != 0 and (goal.reshape(-1)[got.cells[:-1]] == 0).all()
            assert f64(got.cost) == (cost.astype(f64) * got.mask).sum() - f64(cost.reshape(-1)[reached])
            solved += 1
    assert solved >= 4                                                  # (every map's goal cell is a start)


def test_start_index_is_the_highest_non_zero_cell():
    m = np.zeros((4, 5), f32)
    assert PO.start_index(m) == -1
    m[1, 2] = 1
    assert PO.start_index(m) == 7
    m[3, 4] = 0.5
    assert PO.start_index(m) == 19


def test_a_chosen_gradient_flips_the_route_on_3x3_cell_by_cell():
    """start 0, goal 8, every cost 1 but the centre's 0.25: the route is the diagonal 0, 4, 8.  An upstream gradient of +1 on the centre and
    lambda = 4 make the centre cost 4.25: the perturbed route goes round it -- 0, then 1 (the first action among the equals 1 and 3), 5, 8"""
    cost = np.ones((3, 3), f32)
    cost[1, 1] = 0.25
    goal, passable, g = np.zeros((3, 3), f32), np.ones((3, 3), f32), np.zeros((3, 3), f32)
    goal[2, 2] = 1
    g[1, 1] = 1
    fwd = PO.path(cost, goal, passable, 0)
    assert fwd.status == 0 and fwd.cells == [0, 4, 8] and fwd.cost == 1.25
    assert PO.perturbed(cost, g, 4.0, 2.0 ** -10).reshape(-1).tolist() == [1, 1, 1, 1, 4.25, 1, 1, 1, 1]
    grad, st, _, lam = PO.backward(cost, goal, passable, 0, g, 4.0, 2.0 ** -10)
    assert st == 0 and lam.cells == [0, 1, 5, 8] and lam.cost == 3
    assert grad.dtype == f32 and grad.reshape(-1).tolist() == [0, 0.25, 0, 0, -0.25, 0.25, 0, 0, 0]
    # a gradient too small to move the route: an all-zero row
    grad, st, _, lam = PO.backward(cost, goal, passable, 0, g, 0.5, 2.0 ** -10)
    assert st == 0 and lam.cells == [0, 4, 8] and not grad.any()
    # lambda that is no power of two: the factor is fl32(1 / lambda)
    grad, _, _, _ = PO.backward(cost, goal, passable, 0, g, 3.0, 2.0 ** -10)
    assert sorted(set(grad.reshape(-1).tolist())) == [-float(f32(1) / f32(3)), 0, float(f32(1) / f32(3))]


def test_the_clamp_at_min_cost():
    """3x5, start (1,0), goal (1,4), unit costs; a gradient of -1 on three cells of the top row and lambda = 20 would make them cost -19: they
    cost min_cost instead, and the perturbed route takes them"""
    cost, passable, goal, g = np.ones((3, 5), f32), np.ones((3, 5), f32), np.zeros((3, 5), f32), np.zeros((3, 5), f32)
    goal[1, 4] = 1
    g[0, 1:4] = -1
    w = PO.perturbed(cost, g, 20.0, 0.25)
    assert w.dtype == f32 and w[0].tolist() == [1, 0.25, 0.25, 0.25, 1] and (w[1:] == 1).all()
    assert PO.perturbed(cost, g, 20.0, 2.0 ** -10)[0, 2] == f32(2.0 ** -10)
    assert PO.perturbed(cost, g * 0.03, 20.0, 0.25)[0, 2] == f32(f32(f32(20) * f32(-0.03)) + f32(1)) > 0.25   # above the floor: two roundings, no clamp
    grad, st, fwd, lam = PO.backward(cost, goal, passable, 5, g, 20.0, 0.25)
    assert st == 0 and fwd.cells == [5, 6, 7, 8, 9] and lam.cells == [5, 1, 2, 3, 9] and lam.cost == 1.75
    want = np.zeros(15, f32)
    want[[1, 2, 3]], want[[6, 7, 8]] = 0.05, -0.05
    assert np.array_equal(grad.reshape(-1), want)
    _, _, changed, clamped = PO.batch_backward(cost[None], goal[None], passable[None], [5], g[None], 20.0, 0.25)
    assert changed.tolist() == [True] and clamped.tolist() == [True]
    # a NaN is not clamped away: the perturbed solve fails with BAD_COST and the row is all NaN -- on a passable cell only
    g[2, 2] = np.nan
    grad, st, _, _ = PO.backward(cost, goal, passable, 5, g, 20.0, 0.25)
    assert st == PO.STATUS_BAD_COST and np.isnan(grad).all()
    passable[2, 2] = 0
    grad, st, _, _ = PO.backward(cost, goal, passable, 5, g, 20.0, 0.25)
    assert st == 0 and np.array_equal(grad.reshape(-1), want)


def test_failed_maps_have_a_zero_mask_an_infinite_cost_and_a_zero_gradient():
    cost, passable, goal = np.ones((5, 9), f32), np.ones((5, 9), f32), np.zeros((5, 9), f32)
    goal[2, 8] = 1
    walled = passable.copy()
    walled[:, 4] = 0                                                    # a wall between the start and the goal
    plateau = cost.copy()
    plateau[2, 4:8] = 0                                                 # a zero-cost corridor in front of the goal
    nan = cost.copy()
    nan[0, 0] = np.nan
    cases = [(cost, goal, passable, -1, 1), (cost, goal, passable, 45, 1), (cost, goal, walled, 18, 3), (cost, goal, walled, 22, 3),
             (cost, np.zeros_like(goal), passable, 18, 3), (plateau, goal, passable, 18, 11), (nan, goal, passable, 18, 9),
             (nan, goal, passable, -1, 1), (nan, np.zeros_like(goal), passable, 18, 9), (plateau, goal, walled, 18, 3)]
    for c, g, p, n0, status in cases:
        got = PO.path(c, g, p, n0)
        assert got.status == status and not got.mask.any() and np.isposinf(got.cost) and got.cells == [], (n0, status)
        grad, st, _, lam = PO.backward(c, g, p, n0, np.ones((5, 9), f32), 2.0, 0.25)
        assert st == 0 and lam is None and not grad.any()
    ok = PO.path(cost, goal, passable, 18)
    assert ok.status == 0 and ok.cost == 8 and ok.mask.sum() == 9
    assert PO.path(plateau, goal, passable, 26).status == 0            # the goal itself: nothing to chase
    on_wall = PO.path(cost, goal, np.zeros_like(passable), 26)          # a start on a goal on an obstacle: [n0]
    assert on_wall.status == 0 and on_wall.cells == [26] and on_wall.cost == 0
    masks, costs, status = PO.batch(np.stack([cost, plateau, cost]), np.stack([goal] * 3), np.stack([passable, passable, walled]), [18, 18, 18])
    assert status.tolist() == [0, 11, 3] and masks[0].sum() == 9 and not masks[1:].any() and costs.tolist() == [8, np.inf, np.inf]


# ---- 2: header, binding, library ----------------------------------------------------------------------------------------------------------------------
NAMES = ["nastar_path_masks", "nastar_path_masks_abi", "nastar_path_masks_backward", "nastar_path_masks_max_cells"]
ARGS = ["cost", "goal", "passable", "start_idx", "B", "H", "W", "neighbor_mask", "path_out", "path_cost_out", "status_out", "stream"]
BACK_ARGS = ["cost", "goal", "passable", "start_idx", "grad_path", "path_fwd", "status_fwd", "B", "H", "W", "neighbor_mask", "lambda", "min_cost",
             "grad_cost_out", "status_out", "stream"]


def test_eleventh_header_and_path_mask_signatures_agree():
    from neural_astar import _native
    protos = _prototypes("nastar_path_masks.h")
    assert sorted(protos) == sorted(_native.PATH_MASK_SIGNATURES) == NAMES
    for name, (ret, args) in protos.items():
        assert _native.PATH_MASK_SIGNATURES[name] == ret + " " + "".join(k for k, _ in args), name
    assert [n for _, n in protos["nastar_path_masks"][1]] == ARGS
    assert [n for _, n in protos["nastar_path_masks_backward"][1]] == BACK_ARGS
    # a table of its own; nastar.h and the other tables are what they were
    for table in (_native.SIGNATURES, _native.ROUTE_SIGNATURES, _native.FIELD_SIGNATURES, _native.TILED_FIELD_SIGNATURES, _native.FIELD_GRAD_SIGNATURES,
                  _native.FIELD_GRAD_TILED_SIGNATURES, _native.FIELD_ROUTE_SIGNATURES):
        assert not set(_native.PATH_MASK_SIGNATURES) & set(table)
    assert len(_prototypes("nastar.h")) == len(_native.SIGNATURES) == 74 and len(_prototypes("nastar_field_routes.h")) == 5
    new = _defines("nastar_path_masks.h")
    assert new["NASTAR_PATH_MASKS_ABI"] == 1 and "NASTAR_VERSION" not in new and _defines("nastar.h")["NASTAR_VERSION"] == 800
    assert not [k for k in new if k.startswith("NASTAR_ERR_")]      # no new status code: 1, 3, 9, 10 and 11 are the other headers'
    assert (PO.STATUS_BAD_SHAPE, PO.STATUS_UNSOLVABLE, PO.STATUS_BAD_COST, PO.STATUS_PLATEAU) == (
        _native.NASTAR_ERR_BAD_SHAPE, _native.NASTAR_ERR_UNSOLVABLE, _native.NASTAR_ERR_BAD_COST, _native.NASTAR_ERR_PLATEAU)


def test_library_exports_the_path_mask_symbols():
    from neural_astar import _native, ops
    lib = _native.load()
    for sym in NAMES:
        assert hasattr(lib, sym), sym
    assert lib.nastar_path_masks_abi() == 1
    assert lib.nastar_path_masks_max_cells() == ops.PATH_MASKS_MAX_CELLS == lib.nastar_fields_max_cells() == 16384
    assert len(lib.nastar_path_masks.argtypes) == 12 and len(lib.nastar_path_masks_backward.argtypes) == 16
    assert {"shortest_paths", "PathOutput", "path_masks", "path_masks_backward", "PATH_MASKS_MAX_CELLS"} <= set(ops.__all__)


# ---- 3: refusals, made before any HIP call --------------------------------------------------------------------------------------------------------------
def _args(**over):
    p = 0x10000  # never dereferenced: every call below is refused on its arguments
    a = dict(cost=p, goal=p, passable=p, start_idx=p, B=2, H=32, W=32, neighbor_mask=0x1EF, path_out=p, path_cost_out=None, status_out=p, stream=None)
    assert list(a) == ARGS
    a.update(over)
    return a


def _back_args(**over):
    p = 0x10000
    a = dict(cost=p, goal=p, passable=p, start_idx=p, grad_path=p, path_fwd=p, status_fwd=p, B=2, H=32, W=32, neighbor_mask=0x1EF, lambda_=20.0,
             min_cost=2.0 ** -10, grad_cost_out=p, status_out=None, stream=None)
    assert [k.rstrip("_") for k in a] == BACK_ARGS
    a.update(over)
    return a


SHARED_REFUSALS = [
    (dict(cost=None), 5), (dict(goal=None), 5), (dict(passable=None), 5), (dict(start_idx=None), 5),
    (dict(B=0), 1), (dict(H=0), 1), (dict(W=-1), 1), (dict(B=-3), 1),
    (dict(neighbor_mask=0x1FF), 2), (dict(neighbor_mask=0x200), 2),
    (dict(neighbor_mask=0x010, cost=None), 2),                         # the mask is looked at first
    (dict(cost=None, B=0), 5),                                          # a NULL before the shape
    (dict(B=0, H=129, W=128), 1),                                       # the shape before the limit
    (dict(H=129, W=128), 2), (dict(H=1, W=16385), 2), (dict(H=65536, W=65536), 2)]


@pytest.mark.parametrize("over,rc", SHARED_REFUSALS + [(dict(path_out=None), 5), (dict(status_out=None), 5), (dict(path_out=None, H=0), 5)])
def test_path_masks_refuses_bad_arguments_without_a_device(over, rc):
    from neural_astar import _native
    lib = _native.load()
    assert lib.nastar_path_masks(*_args(**over).values()) == rc
    assert lib.nastar_path_masks(*_args(path_cost_out=0x10000, **over).values()) == rc
    assert lib.nastar_last_error() == b""


@pytest.mark.parametrize("over,rc", SHARED_REFUSALS + [
    (dict(grad_path=None), 5), (dict(path_fwd=None), 5), (dict(status_fwd=None), 5), (dict(grad_cost_out=None), 5),
    (dict(lambda_=0.0), 2), (dict(lambda_=-1.0), 2), (dict(lambda_=float("inf")), 2), (dict(lambda_=float("nan")), 2),
    (dict(lambda_=1e-45), 2),                                           # a denormal: its fp32 reciprocal is not finite
    (dict(min_cost=0.0), 2), (dict(min_cost=-0.5), 2), (dict(min_cost=float("inf")), 2), (dict(min_cost=float("nan")), 2),
    (dict(lambda_=0.0, H=129, W=128), 2),
    (dict(lambda_=0.0, B=0), 1), (dict(min_cost=0.0, grad_path=None), 5), (dict(lambda_=float("nan"), neighbor_mask=0x010), 2)])
def test_path_masks_backward_refuses_bad_arguments_without_a_device(over, rc):
    from neural_astar import _native
    lib = _native.load()
    assert lib.nastar_path_masks_backward(*_back_args(**over).values()) == rc
    assert lib.nastar_path_masks_backward(*_back_args(status_out=0x10000, **over).values()) == rc
    assert lib.nastar_last_error() == b""


# ---- 4: Python refusals without a device ------------------------------------------------------------------------------------------------------------------
def test_ops_and_planners_refuse_before_a_launch():
    from neural_astar import ops
    from neural_astar.planner import NeuralAstar, VanillaAstar
    from neural_astar.planner.differentiable_astar import DifferentiableAstar, PathOutput
    assert ops.PathOutput._fields == ("paths", "costs", "status") and PathOutput is ops.PathOutput
    m = torch.ones(2, 1, 8, 8)
    idx = torch.zeros(2, dtype=torch.int32)
    for kw in (dict(), dict(lambda_=20.0)):
        with pytest.raises(RuntimeError, match="HIP device"):
            ops.shortest_paths(m, m, m, m, **kw)
        with pytest.raises(RuntimeError, match="HIP device"):
            DifferentiableAstar().shortest_paths(m, m, m, m, **kw)
        with pytest.raises(RuntimeError, match="HIP device"):
            VanillaAstar().shortest_paths(m, m, m, **kw)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.path_masks(m, m, m, idx)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.path_masks_backward(m, m, m, idx, m, m, idx, 20.0)
    with pytest.raises(ValueError, match="share one"):
        ops.shortest_paths(m, m, torch.ones(2, 1, 8, 9), m)
    with pytest.raises(ValueError, match="must be a"):
        ops.shortest_paths(torch.ones(8, 8), m, m, m)
    with pytest.raises(TypeError, match="float32"):
        ops.shortest_paths(m.double(), m, m.double(), m.double())
    with pytest.raises(ValueError, match="neighbor_mask"):
        ops.shortest_paths(m, m, m, m, neighbor_mask=0x1FF)
    for bad in (torch.ones(2, 3, 8, 8), torch.ones(2, 1, 8, 9), torch.ones(1, 1, 8, 8), torch.zeros(2, 2, dtype=torch.int64), torch.ones(2, 64)):
        with pytest.raises(ValueError, match="start"):
            ops.shortest_paths(m, bad, m, m)
    for bad in (None, [[0]], m.bool()):
        with pytest.raises((TypeError, ValueError), match="start"):
            ops.shortest_paths(m, bad, m, m)
    for bad in (0, 0.0, -1.0, float("inf"), float("nan"), True, "20", 1e-46, 1e39, torch.tensor(20.0)):
        with pytest.raises(ValueError, match="lambda_"):
            ops.shortest_paths(m, m, m, m, lambda_=bad)
        with pytest.raises(ValueError, match="lambda_"):
            NeuralAstar(encoder_arch="CNN").shortest_paths(m, m, m, lambda_=bad)
        with pytest.raises(ValueError, match="lambda_"):
            ops.path_masks_backward(m, m, m, idx, m, m, idx, bad)
    for bad in (0, -0.25, float("inf"), float("nan"), None, False, 1e-46):
        with pytest.raises(ValueError, match="min_cost"):
            ops.shortest_paths(m, m, m, m, min_cost=bad)
        with pytest.raises(ValueError, match="min_cost"):
            NeuralAstar(encoder_arch="CNN").shortest_paths(m, m, m, lambda_=20.0, min_cost=bad)
    huge = torch.ones(1, 1, 1, 1).expand(1, 1, 129, 128)
    for call in (lambda: ops.shortest_paths(huge, huge, huge, huge), lambda: ops.shortest_paths(huge, huge, huge, huge, lambda_=1.0),
                 lambda: ops.path_masks(huge, huge, huge, idx[:1]), lambda: VanillaAstar().shortest_paths(huge, huge, huge)):
        with pytest.raises(NotImplementedError, match="16384"):
            call()


def test_start_maps_become_one_index_per_map():
    from neural_astar import ops
    maps = torch.zeros(3, 1, 4, 5)
    maps[0, 0, 1, 2] = 1
    maps[1, 0, 0, 0] = maps[1, 0, 3, 4] = 0.5                          # two cells: the highest index
    c = torch.ones(3, 1, 4, 5)
    with pytest.raises(RuntimeError, match="HIP device"):              # (the indices are made before the device is looked at)
        ops.path_masks(c, c, c, maps)
    got = ops._start_indices(maps, 3, 4, 5).reshape(3)
    assert got.dtype == torch.int32 and got.tolist() == [7, 19, -1]
    assert [PO.start_index(maps[b, 0].numpy()) for b in range(3)] == [7, 19, -1]


def test_shortest_paths_signatures():
    from neural_astar import ops
    from neural_astar.planner import NeuralAstar, VanillaAstar
    from neural_astar.planner.differentiable_astar import DifferentiableAstar
    sig = inspect.signature(ops.shortest_paths)
    assert list(sig.parameters) == ["cost_maps", "start_maps", "goal_maps", "obstacles_maps", "neighbor_mask", "lambda_", "min_cost"]
    assert sig.parameters["lambda_"].default is None and sig.parameters["min_cost"].default == 2.0 ** -10
    assert "NOT a tuned number" in ops.shortest_paths.__doc__ and "plateau" in ops.shortest_paths.__doc__
    assert list(inspect.signature(DifferentiableAstar.shortest_paths).parameters) == ["self", "cost_maps", "start_maps", "goal_maps", "obstacles_maps",
                                                                                     "lambda_", "min_cost"]
    for cls in (VanillaAstar, NeuralAstar):
        assert list(inspect.signature(cls.shortest_paths).parameters) == ["self", "map_designs", "start_maps", "goal_maps", "lambda_", "min_cost"]
