"""GPU (-m gpu): the exact shortest path as a 0/1 mask and its blackbox gradient (include/nastar_path_masks.h, ``ops.shortest_paths``, the
planners' ``shortest_paths``) against the numpy definition (tests/path_masks_oracle.py, pinned on the CPU by tests/test_path_masks.py).

Every comparison is EXACT: masks and status are integers in value, a path's cost is the field's own bits at the start, and a gradient is 0
or +-fl32(1/lambda) per cell.  The shapes sit at the edges of the three workgroup widths (1024 | 1025 cells, 4096 | 4097) and at the limit
(16384); the inputs of the backward tests are chosen on the CPU, with the definition, so that the perturbed path differs from the forward
one on at least half of the maps and the clamp binds -- both asserted: a backward that changes nothing proves nothing.
"""
import functools

import numpy as np
import pytest
import torch

import fields_oracle as FO
import fields_tiled_oracle as TO
import heuristic_oracle as HO
import path_masks_oracle as PO

pytestmark = pytest.mark.gpu
f32 = np.float32
DIRECTED = 0x0EB  # one of the asymmetric move sets of the neighbour tests
SHAPES = [(1, 1), (1, 9), (7, 5), (32, 32), (25, 41), (64, 64), (17, 241), (128, 128)]
MASKS = [HO.MOORE8, HO.VON_NEUMANN, DIRECTED]


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).to(_dev())  # (a copy: the shared inputs are read-only)


@functools.lru_cache(maxsize=None)
def _maps(H, W, B=3, seed=0, dyadic=False):
    """B seeded maps [B,H,W]: cost U(0.25, 1.25) (``dyadic``: k/64, k in 1..256), passable (about 25 % obstacles; on the 128x128 map, map 2
    is a maze of ``utils.synthetic`` with its own goal), goal: one passable cell per map.  Shared between tests, never modified."""
    from neural_astar.utils import synthetic as syn
    rng = np.random.default_rng([seed, H, W, B])
    passable = (rng.random((B, H, W)) > 0.25).astype(f32)
    goal = np.zeros((B, H, W), f32)
    for b in range(B):
        first = (int(rng.integers(H)), int(rng.integers(W)))
        passable[b][first] = 1
        if b == 2 and (H, W) == (128, 128):
            P = syn.maze_maps(1, H, seed=seed + 1)
            passable[b], first = P.map_designs[0, 0], tuple(np.argwhere(P.goal_maps[0, 0] != 0)[0])
        goal[b][first] = 1
    cost = (rng.integers(1, 257, (B, H, W)) / 64.0).astype(f32) if dyadic else (0.25 + rng.random((B, H, W))).astype(f32)
    for a in (cost, goal, passable):
        a.setflags(write=False)
    return cost, goal, passable


@functools.lru_cache(maxsize=None)
def _starts(H, W, mask, B=3, seed=0, dyadic=False):
    """[B] int32: per map the reachable cell FARTHEST from the goal under ``mask`` (the longest chase); the goal itself where nothing else
    reaches it"""
    cost, goal, passable = _maps(H, W, B, seed, dyadic)
    dist = FO.fields(cost, goal, passable, mask)[0].reshape(B, -1)
    out = np.argmax(np.where(np.isfinite(dist), dist, -1), axis=1).astype(np.int32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _want(H, W, mask, B=3, seed=0, dyadic=False):
    return PO.batch(*_maps(H, W, B, seed, dyadic), _starts(H, W, mask, B, seed, dyadic), mask)


def _forward(cost, goal, passable, starts, mask=None):
    """``ops.path_masks`` (the raw entry: nothing is read back, nothing raises) on device copies -> numpy (masks [B,H,W], costs, status)"""
    from neural_astar import ops
    r = ops.path_masks(_t(cost)[:, None], _t(goal)[:, None], _t(passable)[:, None], _t(np.asarray(starts, np.int32)), neighbor_mask=mask)
    B, H, W = cost.shape
    assert r.paths.dtype == r.costs.dtype == torch.float32 and r.status.dtype == torch.int32
    assert tuple(r.paths.shape) == (B, 1, H, W) and tuple(r.costs.shape) == tuple(r.status.shape) == (B,)
    return r.paths[:, 0].cpu().numpy(), r.costs.cpu().numpy(), r.status.cpu().numpy()


def _backward(cost, goal, passable, starts, grad, lam, min_cost, mask=None, fwd=None):
    """``ops.path_masks`` then ``ops.path_masks_backward`` -> numpy (grad_cost [B,H,W], status of the perturbed solve)"""
    from neural_astar import ops
    c, g, p, s = _t(cost)[:, None], _t(goal)[:, None], _t(passable)[:, None], _t(np.asarray(starts, np.int32))
    r = ops.path_masks(c, g, p, s, neighbor_mask=mask) if fwd is None else fwd
    gc, st = ops.path_masks_backward(c, g, p, s, _t(grad)[:, None], r.paths, r.status, lam, min_cost, neighbor_mask=mask)
    assert gc.dtype == torch.float32 and tuple(gc.shape) == cost.shape and st.dtype == torch.int32
    return gc.cpu().numpy(), st.cpu().numpy()


def _same(got, want, what=""):
    for g, w, name in zip(got, want, ("masks", "costs", "status")):
        assert g.shape == w.shape and g.dtype == w.dtype, f"{what}: {name} is {g.dtype}{g.shape}, the definition {w.dtype}{w.shape}"
        same = g.view(np.uint32) == w.view(np.uint32) if name != "status" else g == w
        assert same.all(), f"{what}: {name} differ in {int((~same).sum())} places, first at {tuple(np.argwhere(~same)[0])}"


def _same_grad(got, want, what=""):
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want)) | ((got == 0) & (want == 0))
    assert got.shape == want.shape and same.all(), f"{what}: gradients differ in {int((~same).sum())} places, first at {tuple(np.argwhere(~same)[0])}"


# ---- forward: the definition, the device composition, the search ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("H,W", SHAPES)
def test_masks_are_the_definitions_and_the_device_composition(H, W, mask):
    from neural_astar import ops
    cost, goal, passable = _maps(H, W)
    starts = _starts(H, W, mask)
    want = _want(H, W, mask)
    assert (want[2] == 0).all() and (H * W < 35 or want[0].sum() > 3 * 3)      # every map is solved, from far away
    _same(_forward(cost, goal, passable, starts, mask), want, f"{H}x{W} {mask:#x}")
    # cost_to_go + field_routes + a scatter: the composition the fused launch replaces
    c, g, p = _t(cost)[:, None], _t(goal)[:, None], _t(passable)[:, None]
    fo = ops.cost_to_go(c, g, p, neighbor_mask=mask, policies=False)
    r = ops.field_routes(fo.dists, g, p, _t(starts)[:, None], neighbor_mask=mask, max_route_len=H * W)
    cell = torch.where(r.routes < 0, H * W, r.routes).long()[:, 0]
    composed = torch.zeros((3, H * W + 1), device=_dev()).scatter_(1, cell, 1.0)[:, :H * W].reshape(3, H, W)
    _same((composed.cpu().numpy(), r.route_costs[:, 0].cpu().numpy(), r.status[:, 0].cpu().numpy()), want, f"{H}x{W} {mask:#x} composed")
    print(f"{H}x{W} {mask:#x}: route cells {want[0].sum((1, 2)).astype(int).tolist()}")


def test_one_map_and_more_maps_than_compute_units():
    for B in (1, 300):
        cost, goal, passable = _maps(7, 5, B)
        starts = _starts(7, 5, HO.MOORE8, B)
        want = _want(7, 5, HO.MOORE8, B)
        _same(_forward(cost, goal, passable, starts), want, f"B={B}")
        assert (want[2] == 0).all()
    cost, goal, passable = _maps(128, 128)
    starts = _starts(128, 128, HO.MOORE8)
    _same(_forward(cost[2:], goal[2:], passable[2:], starts[2:]), tuple(a[2:] for a in _want(128, 128, HO.MOORE8)), "B=1, the maze")


def test_serpentine_128x128_a_chase_of_thousands_of_cells():
    cost, goal, passable, walls = TO.serpentine(128, 128)
    rep = lambda a: np.repeat(a[None], 2, axis=0)  # noqa: E731
    starts = np.array([128 * 128 - 1, 127 * 128], np.int32)
    want = PO.batch(rep(cost), rep(goal), rep(passable), starts)
    assert (want[2] == 0).all() and want[0][0].sum() >= walls * 126 and want[1][0] == want[0][0].sum() - 1
    _same(_forward(rep(cost), rep(goal), rep(passable), starts), want, "serpentine")
    print(f"serpentine 128x128: {int(want[0][0].sum())} route cells")


@pytest.mark.parametrize("H,W", [(7, 5), (32, 32), (25, 41)])
def test_path_cost_is_what_a_dijkstra_mode_search_pays_on_dyadic_costs(H, W):
    """two independent kernels: the search with a zero heuristic and g_ratio 1 pays, along ITS route, what the field says at the start --
    exactly, on costs k/64; and that is the sum of the costs under the mask minus the goal's"""
    from neural_astar.planner.differentiable_astar import DifferentiableAstar
    cost, goal, passable = _maps(H, W, dyadic=True)
    starts = _starts(H, W, HO.MOORE8, dyadic=True)
    masks, costs, status = _forward(cost, goal, passable, starts)
    _same((masks, costs, status), _want(H, W, HO.MOORE8, dyadic=True), f"{H}x{W} dyadic")
    da = DifferentiableAstar(g_ratio=1.0, check_solvable=False).to(_dev()).eval()
    for b in range(3):
        start = np.zeros((1, 1, H, W), f32)
        start.reshape(-1)[starts[b]] = 1
        c, g, p = (_t(a[b:b + 1])[:, None] for a in (cost, goal, passable))
        out = da.plan_routes(c, _t(start), g, p, heuristic_maps=torch.zeros_like(c))  # one map per call: no batch loop rule takes part
        assert int(da.last_status[0]) == 0 and float(out.route_costs[0]) == float(costs[b]), b
        assert float(costs[b]) == float((cost[b].astype(np.float64) * masks[b]).sum() - (cost[b] * goal[b]).sum()), b


# ---- failed maps beside healthy ones ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mixed():
    """9x11, eight maps: 0 and 7 healthy, 1 a walled-in start, 2 a start on an obstacle, 3 no goal, 4 a NaN cost, 5 a zero-cost plateau in
    front of the goal, 6 a start out of range -> (cost, goal, passable, starts, the status of each)"""
    H, W, B = 9, 11, 8
    rng = np.random.default_rng(3)
    cost = (0.25 + rng.random((B, H, W))).astype(f32)
    passable, goal = np.ones((B, H, W), f32), np.zeros((B, H, W), f32)
    goal[:, 4, 10] = 1
    starts = np.full(B, 4 * W, np.int32)                                  # (4, 0)
    passable[1, 3:6, 0:2] = 0
    passable[1, 4, 0] = 1                                                 # walled in: passable, its neighbours obstacles
    passable[2, 4, 0] = 0
    goal[3] = 0
    cost[4, 8, 10] = np.nan
    cost[5, :, 7:10] = 0
    starts[6] = H * W
    for a in (cost, goal, passable, starts):
        a.setflags(write=False)
    return cost, goal, passable, starts, [0, 3, 3, 3, 9, 11, 1, 0]


def test_failed_maps_beside_healthy_ones():
    from neural_astar import ops
    cost, goal, passable, starts, status = _mixed()
    want = PO.batch(cost, goal, passable, starts)
    assert want[2].tolist() == status
    got = _forward(cost, goal, passable, starts)
    _same(got, want, "mixed batch")
    assert not got[0][1:7].any() and np.isposinf(got[1][1:7]).all() and got[0][0].sum() >= 11 and got[0][7].sum() >= 11
    # the same batch through start MAPS: an all-zero map is the start out of range; of two non-zero cells the higher index is the start
    smaps = np.zeros((8, 1, 9 * 11), f32)
    smaps[np.arange(8) != 6, 0, 44] = 1
    smaps[0, 0, 3] = 0.5
    c, g, p, s = _t(cost)[:, None], _t(goal)[:, None], _t(passable)[:, None], _t(smaps.reshape(8, 1, 9, 11))
    with pytest.raises(ValueError, match=r"map\(s\) \[4\]"):               # BAD_COST raises, naming the row
        ops.shortest_paths(c, s, g, p)
    keep = [0, 1, 2, 3, 5, 6, 7]
    out = ops.shortest_paths(c[keep], s[keep], g[keep], p[keep])            # every other code stays in status
    _same((out.paths[:, 0].cpu().numpy(), out.costs.cpu().numpy(), out.status.cpu().numpy()), tuple(a[keep] for a in want), "start maps")
    assert not out.paths.requires_grad
    cg = c[keep].clone().requires_grad_(True)
    with pytest.raises(ValueError, match=r"map\(s\) \[4\].*plateau"):      # a differentiable forward raises for the plateau row (map 5) too
        ops.shortest_paths(cg, s[keep], g[keep], p[keep], lambda_=20.0)
    with pytest.raises(NotImplementedError, match="16384"):
        big = torch.ones((1, 1, 129, 128), device=_dev())
        ops.shortest_paths(big, big, big, big)


def test_forward_failed_maps_get_a_zero_gradient_and_a_nan_upstream_a_nan_row_on_its_map_only():
    cost, goal, passable, starts, status = _mixed()
    rng = np.random.default_rng(4)
    grad = np.where(rng.random(cost.shape) < 0.5, f32(1), f32(-1))
    grad[7, 2, 3] = np.nan                                                # a passable cell of a healthy map
    grad[1, 0, 5] = np.nan                                                # ... and of a map whose forward failed: still a zero row
    want, st, changed, _ = PO.batch_backward(cost, goal, passable, starts, grad, 20.0, 0.25)
    assert st.tolist() == [0, 0, 0, 0, 0, 0, 0, 9] and changed[0] and np.isnan(want[7]).all() and not want[1:7].any()
    got, got_st = _backward(cost, goal, passable, starts, grad, 20.0, 0.25)
    _same_grad(got, want, "mixed batch")
    assert np.array_equal(got_st, st) and np.isnan(got[7]).all() and not np.isnan(got[:7]).any() and not got[1:7].any()
    assert set(np.unique(got[0]).tolist()) == {-0.05000000074505806, 0.0, 0.05000000074505806}


# ---- backward: the raw entry against the definition --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _targets(H, W, mask, B=3):
    """seeded random targets: per map the optimal path of ANOTHER seeded cost map (same obstacles, goal and start) -> grad_path = 1 - 2 target"""
    cost, goal, passable = _maps(H, W, B)
    other = (0.25 + np.random.default_rng([9, H, W, B]).random(cost.shape)).astype(f32)
    target = PO.batch(other, goal, passable, _starts(H, W, mask, B), mask)[0]
    grad = (1 - 2 * target).astype(f32)
    grad.setflags(write=False)
    return grad


@pytest.mark.parametrize("min_cost", [2.0 ** -10, 0.25])
@pytest.mark.parametrize("lam", [0.5, 20.0])
@pytest.mark.parametrize("H,W,mask", [(1, 9, HO.MOORE8), (7, 5, HO.VON_NEUMANN), (32, 32, HO.MOORE8), (25, 41, DIRECTED), (64, 64, HO.VON_NEUMANN),
                                      (17, 241, HO.MOORE8), (128, 128, HO.MOORE8)])
def test_backward_is_the_definition(H, W, mask, lam, min_cost):
    cost, goal, passable = _maps(H, W)
    starts, grad = _starts(H, W, mask), _targets(H, W, mask)
    want, st, changed, clamped = PO.batch_backward(cost, goal, passable, starts, grad, lam, min_cost, mask)
    assert (st == 0).all() and clamped.any(), "the clamp was meant to bind"
    assert H == 1 or changed.sum() * 2 >= len(changed), "the perturbed path was meant to differ from the forward one on half of the maps"
    got, got_st = _backward(cost, goal, passable, starts, grad, lam, min_cost, mask)
    _same_grad(got, want, f"{H}x{W} {mask:#x} lambda {lam} min_cost {min_cost}")
    assert np.array_equal(got_st, st)
    inv = float(f32(1) / f32(lam))
    assert set(np.unique(got).tolist()) <= {-inv, 0.0, inv}
    print(f"{H}x{W} {mask:#x} lambda {lam} min_cost {min_cost}: changed {changed.tolist()}, cells moved {(got != 0).sum((1, 2)).tolist()}")


def test_backward_on_more_maps_than_compute_units():
    B = 300
    cost, goal, passable = _maps(7, 5, B)
    starts, grad = _starts(7, 5, HO.MOORE8, B), _targets(7, 5, HO.MOORE8, B)
    want, st, changed, clamped = PO.batch_backward(cost, goal, passable, starts, grad, 20.0, 2.0 ** -10)
    assert (st == 0).all() and clamped.any() and changed.sum() * 2 >= B
    got, got_st = _backward(cost, goal, passable, starts, grad, 20.0, 2.0 ** -10)
    _same_grad(got, want, "B=300")
    assert np.array_equal(got_st, st)


# ---- autograd, capture, the planners -------------------------------------------------------------------------------------------------------------------------
def test_autograd_through_shortest_paths_is_the_raw_entry():
    from neural_astar import ops
    H, W = 25, 41
    cost, goal, passable = _maps(H, W)
    starts, grad = _starts(H, W, DIRECTED), _targets(H, W, DIRECTED)
    smaps = np.zeros((3, 1, H * W), f32)
    smaps[np.arange(3), 0, starts] = 1
    c, s, g, p = _t(cost)[:, None].requires_grad_(True), _t(smaps.reshape(3, 1, H, W)), _t(goal)[:, None], _t(passable)[:, None]
    out = ops.shortest_paths(c, s, g, p, neighbor_mask=DIRECTED, lambda_=20.0, min_cost=0.25)
    assert out.paths.requires_grad and not out.costs.requires_grad and not out.status.requires_grad
    _same((out.paths[:, 0].detach().cpu().numpy(), out.costs.cpu().numpy(), out.status.cpu().numpy()), _want(H, W, DIRECTED), "differentiable forward")
    (out.paths * _t(grad)[:, None]).sum().backward()
    raw, _ = _backward(cost, goal, passable, starts, grad, 20.0, 0.25, DIRECTED)
    assert tuple(c.grad.shape) == (3, 1, H, W) and raw.any()
    _same_grad(c.grad[:, 0].cpu().numpy(), raw, "autograd")
    # a Hamming loss against the target: d|y - t|/dy is +1 where the path leaves the target, -1 where it misses it, 0 where they agree
    target = _t((1 - grad) / 2)[:, None]
    c2 = _t(cost)[:, None].requires_grad_(True)
    out2 = ops.shortest_paths(c2, s, g, p, neighbor_mask=DIRECTED, lambda_=20.0, min_cost=0.25)
    (out2.paths - target).abs().sum().backward()
    hamming = (out2.paths.detach() - target)[:, 0].cpu().numpy()
    _same_grad(c2.grad[:, 0].cpu().numpy(), _backward(cost, goal, passable, starts, hamming, 20.0, 0.25, DIRECTED)[0], "Hamming loss")
    # without lambda_, and under no_grad: an evaluation call
    assert not ops.shortest_paths(c, s, g, p, neighbor_mask=DIRECTED).paths.requires_grad
    with torch.no_grad():
        assert not ops.shortest_paths(c, s, g, p, neighbor_mask=DIRECTED, lambda_=20.0).paths.requires_grad


def test_forward_and_backward_can_be_captured():
    from neural_astar import ops
    H, W = 32, 32
    cost, goal, passable = _maps(H, W)
    starts, grad = _starts(H, W, HO.MOORE8), _targets(H, W, HO.MOORE8)
    c, g, p, s, up = _t(cost)[:, None], _t(goal)[:, None], _t(passable)[:, None], _t(starts), _t(grad)[:, None]
    want = ops.path_masks(c, g, p, s)
    want_grad, _ = ops.path_masks_backward(c, g, p, s, up, want.paths, want.status, 20.0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = ops.shortest_paths(c, s, g, p)                              # (inside a capture the status is not read)
        got_grad, _ = ops.path_masks_backward(c, g, p, s, up, got.paths, got.status, 20.0)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(got + (got_grad,), want + (want_grad,)):
        assert torch.equal(a, b)
    assert want_grad.any()


def test_vanilla_and_differentiable_planners_are_the_definition():
    from neural_astar.planner import VanillaAstar
    from neural_astar.planner.differentiable_astar import DifferentiableAstar
    from neural_astar.utils import synthetic as syn
    P = syn.maze_maps(3, 32, seed=4)
    m, s, g = (_t(a) for a in P)
    starts = [PO.start_index(P.start_maps[b]) for b in range(3)]
    out = VanillaAstar().to(_dev()).shortest_paths(m, s, g)
    want = PO.batch(P.map_designs[:, 0], P.goal_maps[:, 0], P.map_designs[:, 0], starts)
    _same((out.paths[:, 0].cpu().numpy(), out.costs.cpu().numpy(), out.status.cpu().numpy()), want, "VanillaAstar")
    assert (want[2] == 0).all() and np.array_equal(want[1], want[0].sum((1, 2)) - 1)   # unit costs: the field counts the moves
    da = DifferentiableAstar().to(_dev()).eval()
    with torch.no_grad():
        da.neighbor_filter.copy_(torch.tensor([float((HO.VON_NEUMANN >> i) & 1) for i in range(9)], device=_dev()).reshape(1, 1, 3, 3))
    cost = (0.25 + np.random.default_rng(1).random((3, 1, 32, 32))).astype(f32)
    out = da.shortest_paths(_t(cost), s, g, m)
    want = PO.batch(cost[:, 0], P.goal_maps[:, 0], P.map_designs[:, 0], starts, HO.VON_NEUMANN)
    _same((out.paths[:, 0].cpu().numpy(), out.costs.cpu().numpy(), out.status.cpu().numpy()), want, "DifferentiableAstar, von Neumann")


def test_a_hamming_loss_on_the_paths_trains_the_encoder():
    """the demonstrations are the optimal paths under HIDDEN seeded costs on open maps with many routes, so a freshly initialised encoder
    misses them (asserted); the Hamming loss is a SUM: its gradient per cell is +-1, which lambda = 20 turns into a perturbation far above
    the encoder's costs in (0, 1) -- under a mean over 8192 cells the same lambda would move no path and the gradient would be exactly 0"""
    from neural_astar.planner import NeuralAstar
    from neural_astar.planner.differentiable_astar import DifferentiableAstar
    from neural_astar.utils import synthetic as syn
    P = syn.random_obstacle_maps(8, 32, 32, 0.25, seed=6)
    m, s, g = (_t(a) for a in P)
    hidden = _t((0.25 + np.random.default_rng(6).random((8, 1, 32, 32))).astype(f32))
    demo = DifferentiableAstar().to(_dev()).shortest_paths(hidden, s, g, m)
    assert demo.status.tolist() == [0] * 8
    torch.manual_seed(0)
    planner = NeuralAstar(encoder_arch="CNN").to(_dev()).train()
    out = planner.shortest_paths(m, s, g, lambda_=20.0)
    assert out.paths.requires_grad and out.status.tolist() == [0] * 8
    loss = (out.paths - demo.paths).abs().sum()
    assert float(loss.detach()) > 0, "the fresh encoder was meant to miss the demonstrations"
    loss.backward()
    grads = [q.grad for q in planner.encoder.parameters()]
    assert all(q is not None and bool(torch.isfinite(q).all()) for q in grads) and any(bool(q.any()) for q in grads)
    print(f"encoder route {planner.last_encoder_route}, Hamming loss {float(loss.detach()):.0f}, encoder gradient norms {[round(float(q.norm()), 6) for q in grads[:4]]}")
    with torch.no_grad():
        assert not planner.shortest_paths(m, s, g).paths.requires_grad
