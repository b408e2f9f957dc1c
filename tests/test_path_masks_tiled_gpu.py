"""GPU (-m gpu): the shortest-path mask and its blackbox gradient for maps of up to 1179648 cells (include/nastar_path_masks_tiled.h,
``ops.shortest_paths_tiled``, the planners' ``shortest_paths_tiled``).

Every comparison is EXACT.  Three references: the one-workgroup kernel of include/nastar_path_masks.h on the sizes both take (the same
bits), the numpy definition tests/path_masks_oracle.py above its limit, and the device composition the call replaces (``cost_to_go_tiled``,
``field_routes``, a scatter).  The tile is 64x64 (``ops.fields_tile()``): the shapes sit on it, one cell beyond it, across ragged tiles in
both directions and on single rows and columns.  The inputs of the backward tests are checked on the CPU, with the definition, to move the
path on at least half of the maps and to bind the clamp -- both asserted.
"""
import functools

import numpy as np
import pytest
import torch

import field_routes_oracle as RO
import fields_tiled_oracle as TO
import heuristic_oracle as HO
import path_masks_oracle as PO
from test_path_masks_gpu import DIRECTED, MASKS, _dev, _maps, _same, _same_grad, _starts, _t, _targets, _want

pytestmark = pytest.mark.gpu
f32 = np.float32
TILE = 64
ABOVE = (2 * TILE + 1, 2 * TILE)       # 129x128: the first shape above the one-workgroup limit, 3 x 2 tiles
RAGGED = (2 * TILE + 2, 4 * TILE + 3)  # 130x259: 3 x 5 tiles, ragged in both directions


def test_the_shapes_are_derived_from_the_tile():
    from neural_astar import ops
    assert ops.fields_tile() == (TILE, TILE) and ABOVE[0] * ABOVE[1] > ops.PATH_MASKS_MAX_CELLS


def _dev_maps(cost, goal, passable, starts):
    return _t(cost)[:, None], _t(goal)[:, None], _t(passable)[:, None], _t(np.asarray(starts, np.int32))


def _np(r):
    return r.paths[:, 0].cpu().numpy(), r.costs.cpu().numpy(), r.status.cpu().numpy()


def _forward(cost, goal, passable, starts, mask=None, **kw):
    """``ops.path_masks_tiled`` (the raw entry: nothing raises) on device copies -> numpy (masks [B,H,W], costs, status)"""
    from neural_astar import ops
    r = ops.path_masks_tiled(*_dev_maps(cost, goal, passable, starts), neighbor_mask=mask, **kw)
    B, H, W = cost.shape
    assert r.paths.dtype == r.costs.dtype == torch.float32 and r.status.dtype == torch.int32
    assert tuple(r.paths.shape) == (B, 1, H, W) and tuple(r.costs.shape) == tuple(r.status.shape) == (B,)
    return _np(r)


def _backward(cost, goal, passable, starts, grad, lam, min_cost, mask=None, **kw):
    """``ops.path_masks_tiled`` then ``ops.path_masks_tiled_backward`` -> numpy (grad_cost [B,H,W], status of the perturbed solve)"""
    from neural_astar import ops
    c, g, p, s = _dev_maps(cost, goal, passable, starts)
    r = ops.path_masks_tiled(c, g, p, s, neighbor_mask=mask)
    gc, st = ops.path_masks_tiled_backward(c, g, p, s, _t(grad)[:, None], r.paths, r.status, lam, min_cost, neighbor_mask=mask, **kw)
    assert gc.dtype == torch.float32 and tuple(gc.shape) == cost.shape and st.dtype == torch.int32 and tuple(st.shape) == (len(cost),)
    return gc.cpu().numpy(), st.cpu().numpy()


def _composed(cost, goal, passable, starts, mask=None):
    """``cost_to_go_tiled`` + ``field_routes`` + a scatter: the composition the call replaces -> numpy (masks, costs, status)"""
    from neural_astar import ops
    B, H, W = cost.shape
    c, g, p, s = _dev_maps(cost, goal, passable, starts)
    fo, _ = ops.cost_to_go_tiled(c, g, p, neighbor_mask=mask, policies=False)
    r = ops.field_routes(fo.dists, g, p, s[:, None], neighbor_mask=mask, max_route_len=H * W)
    cell = torch.where(r.routes < 0, H * W, r.routes).long()[:, 0]
    masks = torch.zeros((B, H * W + 1), device=_dev()).scatter_(1, cell, 1.0)[:, :H * W].reshape(B, H, W)
    costs = torch.where(r.status[:, 0] == 0, r.route_costs[:, 0], torch.full_like(r.route_costs[:, 0], float("inf")))
    return masks.cpu().numpy(), costs.cpu().numpy(), r.status[:, 0].cpu().numpy()


def _far_starts(cost, goal, passable, mask=None):
    """[B] int32: per map the reachable cell farthest from the goal, read off the DEVICE field (no numpy relaxation of a large map)"""
    from neural_astar import ops
    fo, _ = ops.cost_to_go_tiled(_t(cost)[:, None], _t(goal)[:, None], _t(passable)[:, None], neighbor_mask=mask, policies=False)
    d = fo.dists.reshape(len(cost), -1)
    return torch.where(torch.isfinite(d), d, torch.full_like(d, -1.0)).argmax(1).to(torch.int32).cpu().numpy()


# ---- 1: the same bits as the one-workgroup kernel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("H,W", [(TILE, TILE), (TILE + 1, TILE + 1), (70, 130), (1, 197), (197, 1), (127, 129)])
def test_same_bits_as_the_one_workgroup_kernel(H, W, mask):
    from neural_astar import ops
    cost, goal, passable = _maps(H, W)
    starts, grad = _starts(H, W, mask), _targets(H, W, mask)
    c, g, p, s = _dev_maps(cost, goal, passable, starts)
    one = ops.path_masks(c, g, p, s, neighbor_mask=mask)
    got = _forward(cost, goal, passable, starts, mask)
    _same(got, _np(one), f"{H}x{W} {mask:#x}")
    assert (got[2] == 0).all() and got[0].sum() >= 3
    for lam, floor in [(20.0, 2.0 ** -10)] + ([(0.5, 0.25)] if (H, W) == (70, 130) else []):
        want, want_st = ops.path_masks_backward(c, g, p, s, _t(grad)[:, None], one.paths, one.status, lam, floor, neighbor_mask=mask)
        gc, st = _backward(cost, goal, passable, starts, grad, lam, floor, mask)
        _same_grad(gc, want.cpu().numpy(), f"{H}x{W} {mask:#x} lambda {lam}")
        assert np.array_equal(st, want_st.cpu().numpy()) and (st == 0).all()
        assert min(H, W) == 1 or gc.any(), "the perturbed path was meant to differ somewhere"


# ---- 2: the definition above the old limit -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _row_maps():
    """1x16385, two maps: map 0 open, the goal at column 8000 and the start at the last cell -- a chase of 8385 cells through 132 tiles;
    map 1 seeded obstacles (short segments)"""
    W = 4 * 64 * 64 + 1
    cost, goal, passable = (a.copy() for a in _maps(1, W, 2))
    starts = _starts(1, W, HO.VON_NEUMANN, 2).copy()
    passable[0], goal[0] = 1, 0
    goal[0, 0, 8000] = 1
    starts[0] = W - 1
    for a in (cost, goal, passable, starts):
        a.setflags(write=False)
    return cost, goal, passable, starts


@pytest.mark.parametrize("H,W,mask", [ABOVE + (HO.MOORE8,), RAGGED + (HO.MOORE8,), RAGGED + (DIRECTED,), (1, 4 * TILE * TILE + 1, HO.VON_NEUMANN)])
def test_masks_are_the_definitions_above_the_old_limit(H, W, mask):
    if H == 1:
        cost, goal, passable, starts = _row_maps()
        want = PO.batch(cost, goal, passable, starts, mask)
        assert want[0][0].sum() == 8385
    else:
        cost, goal, passable = _maps(H, W, 2)
        starts, want = _starts(H, W, mask, 2), _want(H, W, mask, 2)
    assert H * W > 16384 and (want[2] == 0).all() and (want[0].sum((1, 2)) >= 4).all()
    _same(_forward(cost, goal, passable, starts, mask), want, f"{H}x{W} {mask:#x}")
    _same(_composed(cost, goal, passable, starts, mask), want, f"{H}x{W} {mask:#x} composed")
    print(f"{H}x{W} {mask:#x}: route cells {want[0].sum((1, 2)).astype(int).tolist()}")


def test_five_by_seven_tiles_against_the_composition():
    H, W = 300, 400
    cost, goal, passable = _maps(H, W, 2)
    for mask in (HO.MOORE8, DIRECTED):
        starts = _far_starts(cost, goal, passable, mask)
        want = _composed(cost, goal, passable, starts, mask)
        assert (want[2] == 0).all() and (want[0].sum((1, 2)) > 3 * TILE).all()      # every route crosses several tiles
        _same(_forward(cost, goal, passable, starts, mask), want, f"300x400 {mask:#x}")


# ---- 3: a serpentine ------------------------------------------------------------------------------------------------------------------------------------------
def test_serpentine_130x259_a_chase_of_thousands_of_cells_across_tile_borders():
    """the expectation is the route oracle's on the DEVICE field (a numpy relaxation of this map takes 11000 sweeps; the field itself is
    tests/test_fields_tiled_gpu.py's subject): unit costs, so the cost is the number of moves"""
    from neural_astar import ops
    H, W = RAGGED
    cost, goal, passable, walls = TO.serpentine(H, W)
    rep = lambda a: np.repeat(a[None], 2, axis=0)  # noqa: E731
    starts = np.array([H * W - 1, (H - 1) * W], np.int32)
    fo, _ = ops.cost_to_go_tiled(_t(cost)[None, None], _t(goal)[None, None], _t(passable)[None, None], policies=False)
    dist = fo.dists[0, 0].cpu().numpy()
    succ = RO.successors(dist, goal, passable)
    masks, costs = np.zeros((2, H * W), f32), np.zeros(2, f32)
    for b in range(2):
        cells, st = RO.route(dist, goal, succ, int(starts[b]))
        assert st == 0 and len(cells) >= walls * (W - 2) and cells[0] == starts[b] and cells[-1] == 0
        masks[b, cells], costs[b] = 1, len(cells) - 1
    want = (masks.reshape(2, H, W), costs, np.zeros(2, np.int32))
    assert np.array_equal(costs, dist.reshape(-1)[starts]) and abs(int(costs[0]) - int(costs[1])) >= W - 3    # the two ends of the last corridor
    got = _forward(rep(cost), rep(goal), rep(passable), starts)
    _same(got, want, "serpentine")
    _same(_composed(rep(cost), rep(goal), rep(passable), starts), want, "serpentine composed")
    print(f"serpentine {H}x{W}: {int(masks[0].sum())} and {int(masks[1].sum())} route cells, {walls} walls")


# ---- 4: batch sizes ---------------------------------------------------------------------------------------------------------------------------------------------
def test_one_map_and_forty_maps():
    H, W = ABOVE
    cost, goal, passable = _maps(H, W, 2)
    starts, want = _starts(H, W, HO.MOORE8, 2), _want(H, W, HO.MOORE8, 2)
    _same(_forward(cost[1:], goal[1:], passable[1:], starts[1:]), tuple(a[1:] for a in want), "B=1")
    cost, goal, passable = _maps(H, W, 40)
    starts = _far_starts(cost, goal, passable)
    want = _composed(cost, goal, passable, starts)
    assert (want[2] == 0).all() and len({int(n) for n in want[0].sum((1, 2))}) > 20     # forty different routes
    got = _forward(cost, goal, passable, starts)
    _same(got, want, "B=40")
    for b in (0, 17, 39):                                                  # ... and a map alone gives what it gives in the batch
        _same(_forward(cost[b:b + 1], goal[b:b + 1], passable[b:b + 1], starts[b:b + 1]), tuple(a[b:b + 1] for a in got), f"map {b} alone")


# ---- 5: failed maps beside healthy ones ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mixed():
    """129x128, nine maps: 0 and 8 healthy, 1 a walled-in start, 2 a start on an obstacle, 3 no goal, 4 a NaN cost, 5 a zero-cost plateau in
    front of the goal, 6 a start out of range, 7 a negative cost -> (cost, goal, passable, starts, the status of each).  Start (64, 0) and
    goal (64, 127): a route crosses the tile border at column 64"""
    H, W = ABOVE
    B = 9
    rng = np.random.default_rng(5)
    cost = (0.25 + rng.random((B, H, W))).astype(f32)
    passable, goal = np.ones((B, H, W), f32), np.zeros((B, H, W), f32)
    goal[:, 64, 127] = 1
    starts = np.full(B, 64 * W, np.int32)
    passable[1, 63:66, 0:2] = 0
    passable[1, 64, 0] = 1                                                # walled in: passable, its neighbours obstacles
    passable[2, 64, 0] = 0
    goal[3] = 0
    cost[4, 128, 127] = np.nan
    cost[5, :, 120:127] = 0
    starts[6] = H * W
    cost[7, 0, 70] = -0.5
    for a in (cost, goal, passable, starts):
        a.setflags(write=False)
    return cost, goal, passable, starts, [0, 3, 3, 3, 9, 11, 1, 9, 0]


def test_failed_maps_beside_healthy_ones():
    from neural_astar import ops
    cost, goal, passable, starts, status = _mixed()
    want = PO.batch(cost, goal, passable, starts)
    assert want[2].tolist() == status
    got = _forward(cost, goal, passable, starts)
    _same(got, want, "mixed batch")
    assert not got[0][1:8].any() and np.isposinf(got[1][1:8]).all() and got[0][0].sum() >= 128 and got[0][8].sum() >= 128
    for b in (0, 8):                                                      # the healthy neighbours are what they are alone
        _same(_forward(cost[b:b + 1], goal[b:b + 1], passable[b:b + 1], starts[b:b + 1]), tuple(a[b:b + 1] for a in got), f"map {b} alone")
    c, g, p, s = _dev_maps(cost, goal, passable, starts)
    with pytest.raises(ValueError, match=r"map\(s\) \[4, 7\]"):             # BAD_COST raises, naming the rows
        ops.shortest_paths_tiled(c, s, g, p)
    keep = [0, 1, 2, 3, 5, 6, 8]
    out = ops.shortest_paths_tiled(c[keep], s[keep], g[keep], p[keep])      # every other code stays in status
    _same(_np(out), tuple(a[keep] for a in want), "shortest_paths_tiled")
    cg = c[keep].clone().requires_grad_(True)
    with pytest.raises(ValueError, match=r"map\(s\) \[4\].*plateau"):      # a differentiable forward raises for the plateau row (map 5) too
        ops.shortest_paths_tiled(cg, s[keep], g[keep], p[keep], lambda_=20.0)


# ---- 6: max_rounds ------------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _two_reaches():
    """200x300, two maps, the goal at (5, 5).  Map 0 is open and starts at (190, 290), four tiles away in both directions.  Map 1 is passable
    in rows and columns 2..40 only -- nothing it lowers lies on the border of tile (0, 0), so it is quiet after ONE round -- and starts at
    (38, 38)"""
    H, W = 200, 300
    cost = (0.25 + np.random.default_rng(6).random((2, H, W))).astype(f32)
    passable, goal = np.ones((2, H, W), f32), np.zeros((2, H, W), f32)
    passable[1] = 0
    passable[1, 2:41, 2:41] = 1
    goal[:, 5, 5] = 1
    starts = np.array([190 * W + 290, 38 * W + 38], np.int32)
    for a in (cost, goal, passable, starts):
        a.setflags(write=False)
    return cost, goal, passable, starts


def test_max_rounds_cuts_the_far_map_short_and_leaves_the_near_one_alone():
    from neural_astar import ops
    cost, goal, passable, starts = _two_reaches()
    c, g, p, s = _dev_maps(cost, goal, passable, starts)
    full, rounds = ops.path_masks_tiled(c, g, p, s, return_rounds=True)
    assert full.status.tolist() == [0, 0] and 4 <= rounds <= 200 * 300 + 1
    want1 = PO.path(cost[1], goal[1], passable[1], int(starts[1]))
    assert want1.status == 0 and len(want1.cells) >= 34
    cut, rounds1 = ops.path_masks_tiled(c, g, p, s, max_rounds=1, return_rounds=True)
    assert rounds1 == 1 and cut.status.tolist() == [10, 0]
    assert not cut.paths[0].any() and float(cut.costs[0]) == float("inf")
    _same(tuple(a[1:] for a in _np(cut)), (want1.mask[None], np.array([want1.cost], f32), np.zeros(1, np.int32)), "the near map, one round")
    assert torch.equal(cut.paths[1], full.paths[1]) and torch.equal(cut.costs[1:], full.costs[1:])
    enough, n = ops.path_masks_tiled(c, g, p, s, max_rounds=rounds, return_rounds=True)
    assert n == rounds and all(torch.equal(a, b) for a, b in zip(enough, full))


# ---- 7: backward is the definition -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_cost", [2.0 ** -10, 0.25])
@pytest.mark.parametrize("lam", [0.5, 20.0])
@pytest.mark.parametrize("H,W,mask", [ABOVE + (HO.MOORE8,), RAGGED + (DIRECTED,)])
def test_backward_is_the_definition(H, W, mask, lam, min_cost):
    B = 4
    cost, goal, passable = _maps(H, W, B)
    starts, grad = _starts(H, W, mask, B), _targets(H, W, mask, B)
    want, st, changed, clamped = PO.batch_backward(cost, goal, passable, starts, grad, lam, min_cost, mask)
    assert (st == 0).all() and clamped.any(), "the clamp was meant to bind"
    assert changed.sum() * 2 >= B, "the perturbed path was meant to differ from the forward one on half of the maps"
    got, got_st = _backward(cost, goal, passable, starts, grad, lam, min_cost, mask)
    _same_grad(got, want, f"{H}x{W} {mask:#x} lambda {lam} min_cost {min_cost}")
    assert np.array_equal(got_st, st)
    inv = float(f32(1) / f32(lam))
    assert set(np.unique(got).tolist()) <= {-inv, 0.0, inv}
    print(f"{H}x{W} {mask:#x} lambda {lam} min_cost {min_cost}: changed {changed.tolist()}, cells moved {(got != 0).sum((1, 2)).tolist()}")


# ---- 8: row conventions ------------------------------------------------------------------------------------------------------------------------------------------------
def test_forward_failed_maps_get_a_zero_row_and_a_nan_upstream_a_nan_row_on_its_map_only():
    cost, goal, passable, starts, status = _mixed()
    rng = np.random.default_rng(4)
    grad = np.where(rng.random(cost.shape) < 0.5, f32(1), f32(-1))
    grad[8, 2, 3] = np.nan                                                # a passable cell of a healthy map
    grad[1, 0, 5] = np.nan                                                # ... and of a map whose forward failed: still a zero row
    want, st, changed, _ = PO.batch_backward(cost, goal, passable, starts, grad, 20.0, 0.25)
    assert st.tolist() == [0] * 8 + [9] and changed[0] and np.isnan(want[8]).all() and not want[1:8].any()
    got, got_st = _backward(cost, goal, passable, starts, grad, 20.0, 0.25)
    _same_grad(got, want, "mixed batch")
    assert np.array_equal(got_st, st) and np.isnan(got[8]).all() and not np.isnan(got[:8]).any() and not got[1:8].any()
    assert set(np.unique(got[0]).tolist()) == {-0.05000000074505806, 0.0, 0.05000000074505806}


def test_a_perturbed_solve_cut_short_gets_a_nan_row_and_status_10():
    cost, goal, passable, starts = _two_reaches()
    grad = np.where(np.random.default_rng(7).random(cost.shape) < 0.5, f32(1), f32(-1))
    want, st, _, _ = PO.batch_backward(cost[1:], goal[1:], passable[1:], starts[1:], grad[1:], 0.5, 0.25)
    assert st.tolist() == [0]
    got, got_st = _backward(cost, goal, passable, starts, grad, 0.5, 0.25, max_rounds=1)
    assert got_st.tolist() == [10, 0] and np.isnan(got[0]).all()
    _same_grad(got[1:], want, "the near map, one round")
    whole, whole_st = _backward(cost, goal, passable, starts, grad, 0.5, 0.25)
    assert whole_st.tolist() == [0, 0] and not np.isnan(whole).any() and whole[0].any()
    _same_grad(whole[1:], want, "the near map")


# ---- 9: autograd and the planners ------------------------------------------------------------------------------------------------------------------------------------------
def test_autograd_through_shortest_paths_tiled_is_the_raw_entry():
    from neural_astar import ops
    H, W = ABOVE
    B = 4
    cost, goal, passable = _maps(H, W, B)
    starts, grad = _starts(H, W, HO.MOORE8, B), _targets(H, W, HO.MOORE8, B)
    smaps = np.zeros((B, 1, H * W), f32)
    smaps[np.arange(B), 0, starts] = 1
    c, s, g, p = _t(cost)[:, None].requires_grad_(True), _t(smaps.reshape(B, 1, H, W)), _t(goal)[:, None], _t(passable)[:, None]
    out = ops.shortest_paths_tiled(c, s, g, p, lambda_=20.0, min_cost=0.25)
    assert out.paths.requires_grad and not out.costs.requires_grad and not out.status.requires_grad
    _same(_np(ops.PathOutput(out.paths.detach(), out.costs, out.status)), PO.batch(cost, goal, passable, starts), "differentiable forward")
    (out.paths * _t(grad)[:, None]).sum().backward()
    raw, _ = _backward(cost, goal, passable, starts, grad, 20.0, 0.25)
    assert tuple(c.grad.shape) == (B, 1, H, W) and raw.any()
    _same_grad(c.grad[:, 0].cpu().numpy(), raw, "autograd")
    # a multi-channel cost tensor: channel 0 is the cost map, and the gradient lands there
    c2 = torch.stack([_t(cost), torch.full((B, H, W), 7.0, device=_dev())], 1).requires_grad_(True)
    out2 = ops.shortest_paths_tiled(c2, s, g, p, lambda_=20.0, min_cost=0.25)
    assert torch.equal(out2.paths, out.paths)
    (out2.paths * _t(grad)[:, None]).sum().backward()
    assert tuple(c2.grad.shape) == (B, 2, H, W) and not c2.grad[:, 1].any()
    _same_grad(c2.grad[:, 0].cpu().numpy(), raw, "autograd, two channels")
    # without lambda_, and under no_grad: an evaluation call
    assert not ops.shortest_paths_tiled(c, s, g, p).paths.requires_grad
    with torch.no_grad():
        assert not ops.shortest_paths_tiled(c, s, g, p, lambda_=20.0).paths.requires_grad


def test_vanilla_and_differentiable_planners_are_the_definition():
    from neural_astar.planner import VanillaAstar
    from neural_astar.planner.differentiable_astar import DifferentiableAstar
    H, W = ABOVE
    rng = np.random.default_rng(9)
    m = (rng.random((2, 1, H, W)) > 0.2).astype(f32)
    s, g = np.zeros_like(m), np.zeros_like(m)
    m[:, 0, 3, 4] = m[:, 0, 120, 100] = 1
    s[:, 0, 3, 4] = g[:, 0, 120, 100] = 1
    starts = [3 * W + 4] * 2
    out = VanillaAstar().to(_dev()).shortest_paths_tiled(_t(m), _t(s), _t(g))
    want = PO.batch(m[:, 0], g[:, 0], m[:, 0], starts)
    _same(_np(out), want, "VanillaAstar")
    assert (want[2] == 0).all() and np.array_equal(want[1], want[0].sum((1, 2)) - 1)   # unit costs: the field counts the moves
    da = DifferentiableAstar().to(_dev()).eval()
    with torch.no_grad():
        da.neighbor_filter.copy_(torch.tensor([float((HO.VON_NEUMANN >> i) & 1) for i in range(9)], device=_dev()).reshape(1, 1, 3, 3))
    cost = (0.25 + rng.random((2, 1, H, W))).astype(f32)
    out = da.shortest_paths_tiled(_t(cost), _t(s), _t(g), _t(m))
    want = PO.batch(cost[:, 0], g[:, 0], m[:, 0], starts, HO.VON_NEUMANN)
    _same(_np(out), want, "DifferentiableAstar, von Neumann")
    assert (want[2] == 0).all()


# ---- 10: capture refusal and streams ------------------------------------------------------------------------------------------------------------------------------------------
def test_capture_is_refused_before_any_launch():
    from neural_astar import ops
    H, W = ABOVE
    cost, goal, passable = _maps(H, W, 2)
    c, g, p, s = _dev_maps(cost, goal, passable, _starts(H, W, HO.MOORE8, 2))
    want = ops.path_masks_tiled(c, g, p, s)
    cg = c.clone().requires_grad_(True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        marker = g + 1.0                                                  # something the capture does hold
        for call in (lambda: ops.shortest_paths_tiled(c, s, g, p), lambda: ops.shortest_paths_tiled(cg, s, g, p, lambda_=20.0),
                     lambda: ops.path_masks_tiled(c, g, p, s),
                     lambda: ops.path_masks_tiled_backward(c, g, p, s, want.paths, want.paths, want.status, 20.0)):
            with pytest.raises(RuntimeError, match="cannot be captured"):
                call()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(marker, g + 1.0)
    again = ops.path_masks_tiled(c, g, p, s)                              # and the call works as before afterwards
    assert all(torch.equal(a, b) for a, b in zip(again, want))


def test_non_default_stream_with_inputs_produced_on_it():
    from neural_astar import ops
    H, W = ABOVE
    cost, goal, passable = _maps(H, W, 2)
    starts, grad = _starts(H, W, HO.MOORE8, 2), _targets(H, W, HO.MOORE8, 2)
    c, g, p, s = _dev_maps(cost, goal, passable, starts)
    base = _t(grad)[:, None]
    want = ops.path_masks_tiled(c, g, p, s)
    want_grad, _ = ops.path_masks_tiled_backward(c, g, p, s, base, want.paths, want.status, 20.0)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=_dev())
    with torch.cuda.stream(side):
        filler = torch.randn(2048, 2048, device=_dev())
        for _ in range(8):                       # work queued ahead of the inputs on the same stream
            filler = filler @ filler * 1e-3
        c2 = c * 2.0 - c                         # == c bit for bit, produced on `side` behind the filler
        up = base * 2.0 - base
        got = ops.path_masks_tiled(c2, g, p, s)  # every launch, copy and wait of the calls is on `side`
        got_grad, st = ops.path_masks_tiled_backward(c2, g, p, s, up, got.paths, got.status, 20.0)
    side.synchronize()
    assert st.tolist() == [0, 0] and all(torch.equal(a, b) for a, b in zip(got, want)) and torch.equal(got_grad, want_grad) and bool(want_grad.any())


# ---- 11: reproducibility ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits():
    H, W = RAGGED
    B = 4
    cost, goal, passable = _maps(H, W, B)
    starts, grad = _starts(H, W, DIRECTED, B), _targets(H, W, DIRECTED, B)
    a, b = _forward(cost, goal, passable, starts, DIRECTED), _forward(cost, goal, passable, starts, DIRECTED)
    _same(a, b, "two forward calls")
    ga, gb = _backward(cost, goal, passable, starts, grad, 20.0, 2.0 ** -10, DIRECTED), _backward(cost, goal, passable, starts, grad, 20.0, 2.0 ** -10, DIRECTED)
    assert np.array_equal(ga[0].view(np.uint32), gb[0].view(np.uint32)) and np.array_equal(ga[1], gb[1]) and ga[0].any()


# ---- 12: a loss on the path trains the encoder above the old limit -----------------------------------------------------------------------------------------------------------
def test_a_hamming_loss_on_the_paths_trains_the_encoder_above_the_old_limit():
    """as tests/test_path_masks_gpu.py's training test, on 2 maps of 129x128: the demonstrations are the optimal paths under HIDDEN seeded
    costs, the Hamming loss is a SUM (its gradient per cell is +-1, which lambda = 20 turns into a perturbation far above the encoder's
    costs in (0, 1))"""
    from neural_astar.planner import NeuralAstar
    from neural_astar.planner.differentiable_astar import DifferentiableAstar
    H, W = ABOVE
    rng = np.random.default_rng(12)
    m = (rng.random((2, 1, H, W)) > 0.2).astype(f32)
    s, g = np.zeros_like(m), np.zeros_like(m)
    m[:, 0, 3, 4] = m[:, 0, 120, 100] = 1
    s[:, 0, 3, 4] = g[:, 0, 120, 100] = 1
    hidden = _t((0.25 + rng.random((2, 1, H, W))).astype(f32))
    m, s, g = _t(m), _t(s), _t(g)
    demo = DifferentiableAstar().to(_dev()).shortest_paths_tiled(hidden, s, g, m)
    assert demo.status.tolist() == [0, 0]
    torch.manual_seed(0)
    planner = NeuralAstar(encoder_arch="CNN").to(_dev()).train()
    out = planner.shortest_paths_tiled(m, s, g, lambda_=20.0)
    assert out.paths.requires_grad and out.status.tolist() == [0, 0]
    loss = (out.paths - demo.paths).abs().sum()
    assert float(loss.detach()) > 0, "the fresh encoder was meant to miss the demonstrations"
    loss.backward()
    grads = [q.grad for q in planner.encoder.parameters()]
    assert grads and all(q is not None and bool(torch.isfinite(q).all()) for q in grads) and any(bool(q.any()) for q in grads)
    print(f"encoder route {planner.last_encoder_route}, Hamming loss {float(loss.detach()):.0f}")
    with torch.no_grad():
        assert not planner.shortest_paths_tiled(m, s, g).paths.requires_grad
