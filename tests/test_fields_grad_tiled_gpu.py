"""GPU (-m gpu): the gradient of the cost-to-go field for maps of up to 1024x1152 (include/nastar_fields_grad_tiled.h,
``ops.fields_backward_tiled``, ``ops.cost_to_go_tiled(..., differentiable=True)``).

Two references.  On the sizes both take, the one-workgroup kernel of item 6g (``ops.fields_backward``): the same BITS, ``torch.equal``.
Above them the numpy float64 definition (tests/fields_grad_oracle.py) at 6g's derived tolerance, |got - ref| <= 2^-23 |ref| + 1e-9 sum|G|
over the live cells of the map: one fp32 rounding at the store (2^-24 relative) doubled, and a ceiling for what the ORDER of an fp64
accumulation can change -- at 130x259 at most 33,670 addends x 2^-53 sum|G| < 4e-12 sum|G|, so the ceiling carries over.  Cells that are not
live are exactly 0.0.  Costs are U(0.5, 1.5): no addition is absorbed at these sizes and no map has a plateau -- asserted on the definition.

The shapes are the smallest at which the tiling can go wrong: one tile (64x64), ragged edges and two tiles in each direction (65x65,
70x130, 127x129, 129x128), one row / one column of tiles (1x197, 197x1), one tile with all eight neighbours (130x259: 3 x 5 tiles).
"""
import functools

import numpy as np
import pytest
import torch

import fields_grad_oracle as GO
import heuristic_oracle as HO
from test_fields_grad_gpu import _case, _close, _serpentine
from test_fields_grad_tiled import ORDER_CASES, _order_case

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
DIRECTED = 0x0EB  # no (1,-1) and no (-1,-1) move: the child sets are not symmetric
MASKS = [HO.MOORE8, HO.VON_NEUMANN, DIRECTED]


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).to(_dev())  # (a copy: the shared inputs are read-only)


@functools.lru_cache(maxsize=None)
def _maps(B, H, W, seed=0):
    """B seeded maps [B,H,W]: cost U(0.5, 1.5), one goal on a passable cell, about 30 % obstacles, upstream gradient N(0, 1).  Shared
    between tests, never modified."""
    rng = np.random.default_rng([seed, B, H, W])
    passable = (rng.random((B, H, W)) > 0.3).astype(f32)
    goal = np.zeros((B, H, W), f32)
    for b in range(B):
        gy, gx = int(rng.integers(H)), int(rng.integers(W))
        goal[b, gy, gx] = passable[b, gy, gx] = 1
    cost = (0.5 + rng.random((B, H, W))).astype(f32)
    G = rng.standard_normal((B, H, W)).astype(f32)
    for a in (cost, goal, passable, G):
        a.setflags(write=False)
    return cost, goal, passable, G


@functools.lru_cache(maxsize=None)
def _refs(B, H, W, mask=HO.MOORE8, seed=0):
    cost, goal, passable, G = _maps(B, H, W, seed)
    refs = GO.field_grads(cost, goal, passable, G, mask)
    assert all(r.status == 0 for r in refs), "U(0.5, 1.5) costs have no plateau at these sizes"
    return refs


def _field(cost, goal, passable, mask=None, policies=False):
    from neural_astar import ops
    return ops.cost_to_go_tiled(_t(cost)[:, None], _t(goal)[:, None], _t(passable)[:, None], neighbor_mask=mask, policies=policies)[0]


def _tiled(dists, goal, passable, G, mask=None, max_rounds=None):
    """the raw entry point -> (grad_cost [B,H,W] tensor, status list, rounds, visits list)"""
    from neural_astar import ops
    B = dists.shape[0]
    visits = torch.full((B,), -7, dtype=torch.int32, device=_dev())
    grad, status, rounds = ops.fields_backward_tiled(dists, _t(goal), _t(passable), _t(G), neighbor_mask=mask, max_rounds=max_rounds, visits_out=visits)
    assert grad.dtype == torch.float32 and tuple(grad.shape) == (B,) + tuple(dists.shape[-2:]) and not grad.requires_grad
    return grad, status.tolist(), rounds, visits.tolist()


def _live_tiles(d, goal):
    """per map: the 64x64 tiles that hold a live cell"""
    live = np.isfinite(d) & (goal == 0)
    B, H, W = live.shape
    return [sum(bool(live[b, y:y + 64, x:x + 64].any()) for y in range(0, H, 64) for x in range(0, W, 64)) for b in range(B)]


# ---- the same bits as the one-workgroup kernel -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("H,W", [(64, 64), (65, 65), (70, 130), (1, 197), (197, 1), (127, 129)])
def test_same_bits_as_the_one_workgroup_kernel(H, W, mask):
    from neural_astar import ops
    for B in (1, 7):
        cost, goal, passable, G = _maps(B, H, W)
        fo = ops.cost_to_go(_t(cost)[:, None], _t(goal)[:, None], _t(passable)[:, None], neighbor_mask=mask, policies=False)
        want, want_st = ops.fields_backward(fo.dists, _t(goal), _t(passable), _t(G), neighbor_mask=mask)
        got, st, rounds, visits = _tiled(fo.dists, goal, passable, G, mask)
        assert st == want_st.tolist() == [0] * B
        assert torch.equal(got, want) and (H * W < 4096 or bool(got.any())), f"{H}x{W} B={B} mask {mask:#x}"
        tiles = _live_tiles(fo.dists[:, 0].cpu().numpy(), goal)
        assert rounds >= 1 and all(v >= t for v, t in zip(visits, tiles)), (rounds, visits, tiles)
        if H * W == 4096:
            assert rounds == 1 and visits == tiles                    # one tile: one visit (none for a walled-in goal: no live cell)


# ---- the summation order itself: both kernels against the in-order evaluation, on a G that shows the order ------------------------------------------
@pytest.mark.parametrize("H,W,mask", ORDER_CASES)
def test_gradient_bits_are_the_in_order_sum(H, W, mask):
    """20x45: one wavefront (T = 64); 70x130: T = 1024, four ragged tiles.  G in {+2^60, -2^60, 1.0}: a changed order of the children changes
    fp32 cells of the result (tests/test_fields_grad_tiled.py::test_the_order_pin_sees_a_reversed_child_order), which a Gaussian G hides."""
    from neural_astar import ops
    goal, passable, dist, G, want = _order_case(H, W, mask)
    d, g, p, up = _t(dist), _t(goal), _t(passable), _t(G)
    one, st1 = ops.fields_backward(d, g, p, up, neighbor_mask=mask)
    tiled, st2, rounds = ops.fields_backward_tiled(d, g, p, up, neighbor_mask=mask)
    assert st1.tolist() == st2.tolist() == [0, 0] and rounds >= 1
    for name, got in (("fields_backward", one), ("fields_backward_tiled", tiled)):
        got = got.cpu().numpy()
        differ = int((got.view(np.uint32) != want.view(np.uint32)).sum())
        print(f"{H}x{W} {hex(mask)} {name}: {differ} of {want.size} fp32 cells differ from the in-order sum")
        assert got.tobytes() == want.tobytes(), name


# ---- above the old limit: the definition ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,mask", [(129, 128, HO.MOORE8), (130, 259, HO.MOORE8), (130, 259, DIRECTED)])
def test_oracle_parity_above_the_old_limit(H, W, mask):
    B = 2
    cost, goal, passable, G = _maps(B, H, W)
    refs = _refs(B, H, W, mask)
    fo = _field(cost, goal, passable, mask)
    assert np.array_equal(fo.dists[:, 0].cpu().numpy(), np.stack([r.dist for r in refs]))
    got, st, rounds, visits = _tiled(fo.dists, goal, passable, G, mask)
    assert st == [0] * B and 1 <= rounds <= H * W + 1
    _close(got.cpu().numpy(), refs, G, f"{H}x{W} mask {mask:#x}: {rounds} rounds, visits {visits}")
    assert max(int(r.hops.max()) for r in refs) > 64                  # routes longer than a tile is wide


def test_nearest_of_three_goals_a_goal_on_an_obstacle_and_what_is_not_live():
    from neural_astar import ops
    H, W = 70, 130
    cost, goal, passable, G = _case(H, W, 3, 1, True)                 # item 6g's case: 3 maps, 3 goals each, map 0 with one on an obstacle
    assert ((goal[0] != 0) & (passable[0] == 0)).any() and (goal != 0).reshape(3, -1).sum(1).max() >= 3
    refs = GO.field_grads(cost, goal, passable, G)
    assert all(r.status == 0 and not r.live[goal[b] != 0].any() for b, r in enumerate(refs))
    live = np.stack([r.live for r in refs])
    poison = np.where(live, G, f32(np.nan))                           # NaN on goals, obstacles and unreachable cells ...
    poison[~live & (passable != 0)] = f32(np.inf)                     # ... and inf on the passable ones among them
    assert np.isnan(poison).sum() > 100 and np.isinf(poison).sum() >= 3
    fo = _field(cost, goal, passable)
    assert np.array_equal(fo.dists[:, 0].cpu().numpy(), np.stack([r.dist for r in refs]))
    got, st, _, _ = _tiled(fo.dists, goal, passable, poison)
    assert st == [0, 0, 0] and bool(torch.isfinite(got).all())
    _close(got.cpu().numpy(), refs, G, "three goals, poisoned dead cells")
    want, _ = ops.fields_backward(fo.dists, _t(goal), _t(passable), _t(G))
    assert torch.equal(got, want)


# ---- a forest about 4600 edges high, across tile borders all the way -------------------------------------------------------------------------------------
def test_serpentine_subtree_sizes_are_exact_and_too_few_rounds_give_zeros():
    H, W = 70, 130
    corridor, path = _serpentine(H, W, False)
    easy = np.zeros((H, W), f32)
    easy[5:25, 5:25] = 1                                              # every live cell and every successor inside one tile
    passable = np.stack([corridor, easy])
    goal = np.zeros((2, H, W), f32)
    goal[0].reshape(-1)[path[0]] = 1
    goal[1, 10, 10] = 1
    want = np.zeros(H * W, f32)
    want[path[1:]] = np.arange(len(path) - 1, 0, -1)
    assert len(path) == 35 * 130 + 35 and want.max() == 4584 < 2 ** 24
    fo = _field(passable, goal, passable, HO.VON_NEUMANN)             # unit costs: D is the number of moves
    assert np.array_equal(fo.dists[0, 0].cpu().numpy().reshape(-1)[path], np.arange(len(path), dtype=f32))
    ones = np.ones((2, H, W), f32)
    got, st, rounds, visits = _tiled(fo.dists, goal, passable, ones, HO.VON_NEUMANN)
    assert st == [0, 0] and np.array_equal(got[0].cpu().numpy().reshape(-1), want)
    print(f"70x130 serpentine, forest height {len(path) - 2}: {rounds} rounds, visits {visits}")
    assert 35 <= rounds <= H * W + 1 and visits[1] == 1               # every corridor crosses the two column borders
    ref = GO.field_grad(easy, goal[1], easy, ones[1], HO.VON_NEUMANN)
    assert np.array_equal(got[1].cpu().numpy(), ref.grad) and ref.grad.max() > 20
    cut, st, r2, _ = _tiled(fo.dists, goal, passable, ones, HO.VON_NEUMANN, max_rounds=2)
    assert st == [10, 0] and r2 == 2 and not bool(cut[0].any())       # a partial subtree sum is a bound of nothing: all zeros
    assert torch.equal(cut[1], got[1])                                # the easy map of the same batch is computed


# ---- against a kernel the tree already trusts: the policy roll-out ------------------------------------------------------------------------------------------
def test_one_hot_gradient_is_the_policy_rollout_across_tile_borders():
    from neural_astar import _native
    H, W = 130, 259
    # map 0: unit costs, no obstacle, the goal at (0, 0): from (129, 258) the policy walks left to the diagonal, then along it -- through
    # the corners (128,128)->(127,127) and (64,64)->(63,63); map 1: a seeded map, the farthest live cell
    cost, goal, passable, _ = (np.array(a) for a in _maps(2, H, W))
    cost[0], passable[0], goal[0] = 1, 1, 0
    goal[0, 0, 0] = 1
    fo = _field(cost, goal, passable, policies=True)
    d = fo.dists[:, 0].cpu().numpy()
    far = int(np.where(np.isfinite(d[1]) & (goal[1] == 0), d[1], -1).argmax())
    starts = np.array([129 * W + 258, far], np.int32)
    G = np.zeros((2, H * W), f32)
    G[[0, 1], starts] = 1
    got, st, rounds, _ = _tiled(fo.dists, goal, passable, G.reshape(2, H, W))
    assert st == [0, 0]
    si, gi = _t(starts), _t(goal.reshape(2, -1).argmax(1).astype(np.int32))
    trajs = torch.empty((2, 1, H, W), dtype=torch.float32, device=_dev())
    rs = torch.empty((2,), dtype=torch.int32, device=_dev())
    rc = _native.load().nastar_policy_rollout(fo.policies.data_ptr(), si.data_ptr(), gi.data_ptr(), 2, 1, 8, H, W, trajs.data_ptr(), rs.data_ptr(),
                                              torch.cuda.current_stream(_dev()).cuda_stream)
    assert rc == 0 and rs.tolist() == [0, 0]
    assert torch.equal(got, trajs[:, 0])
    t0 = got[0].cpu().numpy()
    assert t0[129, 129:].all() and all(t0[k, k] == 1 for k in range(1, 130)) and t0.sum() == 258 and t0[0, 0] == 0
    ys, xs = np.nonzero(got[1].cpu().numpy())
    crossed = len(set(zip((ys // 64).tolist(), (xs // 64).tolist())))
    print(f"one-hot roll-outs: {rounds} rounds; map 1 runs {len(ys)} cells through {crossed} tiles")
    assert crossed >= 2 and rounds >= 3


# ---- the identity that ties the gradient to the field ---------------------------------------------------------------------------------------------------------
def test_gradient_times_cost_sums_to_the_field():
    """G = 1 on live cells: every cell pays its cost once per roll-out through it, so sum(grad_cost * cost) is the sum of D over the live
    cells -- up to the forward's roundings, one per hop: hops_max * 2^-24 relative (item 6g)"""
    H, W = 70, 130
    cost, goal, passable, _ = _maps(2, H, W)
    refs = _refs(2, H, W)
    fo = _field(cost, goal, passable)
    got, st, _, _ = _tiled(fo.dists, goal, passable, np.ones((2, H, W), f32))
    got, d = got.cpu().numpy(), fo.dists[:, 0].cpu().numpy()
    assert st == [0, 0]
    for b, r in enumerate(refs):
        lhs = float((got[b].astype(f64) * cost[b].astype(f64)).sum())
        rhs = float(d[b][r.live].astype(f64).sum())
        print(f"{H}x{W} map {b}: sum(grad * cost) = {lhs!r}, sum(D) = {rhs!r}, hops_max {int(r.hops.max())}")
        assert np.array_equal(got[b], np.round(got[b])) and abs(lhs - rhs) <= int(r.hops.max()) * 2.0 ** -24 * rhs


def test_two_calls_give_the_same_bits():
    cost, goal, passable, G = _maps(2, 130, 259)
    fo = _field(cost, goal, passable)
    a, sa, ra, va = _tiled(fo.dists, goal, passable, G)
    b, sb, rb, vb = _tiled(fo.dists, goal, passable, G)
    assert torch.equal(a, b) and bool(a.any()) and sa == sb == [0, 0]
    tiles = _live_tiles(fo.dists[:, 0].cpu().numpy(), goal)
    print(f"130x259: rounds {ra} / {rb}, visits {va} / {vb}, tiles with a live cell {tiles}")
    for rounds, visits in ((ra, va), (rb, vb)):
        assert 1 <= rounds <= 130 * 259 + 1 and all(t <= v <= 15 * rounds for v, t in zip(visits, tiles))


# ---- statuses: four maps, four stories, one call --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _status_batch():
    """65x65: map 0 ordinary; map 1 without a goal; map 2 with a zero-cost strip; map 3 ordinary"""
    cost, goal, passable, G = (np.array(a) for a in _maps(4, 65, 65, seed=2))
    goal[1] = 0
    y, x = np.argwhere(goal[2] != 0)[0]
    xs = slice(max(0, x - 3), min(65, x + 4))
    passable[2, y, xs] = 1
    cost[2, y, xs] = 0
    return cost, goal, passable, G


def test_statuses_in_one_batch():
    cost, goal, passable, G = _status_batch()
    refs = GO.field_grads(cost, goal, passable, G)
    assert [r.status for r in refs] == [0, 0, 11, 0] and not refs[1].live.any() and refs[3].live.sum() > 50
    fo = _field(cost, goal, passable)
    assert fo.status.tolist() == [0, 3, 0, 0]
    got, st, _, visits = _tiled(fo.dists, goal, passable, G)
    assert st == [0, 0, 11, 0] and visits[1] == 0 and visits[2] == 0 and visits[0] >= 1 and visits[3] >= 1
    got = got.cpu().numpy()
    assert not got[1].any() and not got[2].any()
    _close(got[[0, 3]], [refs[0], refs[3]], G[[0, 3]], "statuses")
    alone, st, _, _ = _tiled(fo.dists[3:4], goal[3:4], passable[3:4], G[3:4])   # the others leave no trace in map 3
    assert st == [0] and np.array_equal(alone[0].cpu().numpy(), got[3])


# ---- autograd ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_autograd_is_the_raw_entry_point():
    from neural_astar import ops
    H, W = 70, 130
    cost, goal, passable, G = _maps(2, H, W)
    c, g, p, w = (_t(a)[:, None] for a in (cost, goal, passable, G))
    c.requires_grad_(True)
    g.requires_grad_(True)
    p.requires_grad_(True)
    plain, rounds = ops.cost_to_go_tiled(c, g, p)
    assert not plain.dists.requires_grad and plain.dists.grad_fn is None     # the default is today's call
    out, rounds2 = ops.cost_to_go_tiled(c, g, p, differentiable=True)
    assert rounds >= 1 and rounds2 >= 1
    assert out.dists.requires_grad and not out.policies.requires_grad and not out.status.requires_grad
    assert torch.equal(out.dists, plain.dists) and torch.equal(out.policies, plain.policies) and torch.equal(out.status, plain.status)
    fin = torch.isfinite(out.dists)
    (out.dists[fin] * w[fin]).sum().backward()
    raw, st, _ = ops.fields_backward_tiled(plain.dists, g.detach(), p.detach(), torch.where(fin, w, torch.zeros_like(w)))
    assert st.tolist() == [0, 0]
    assert tuple(c.grad.shape) == (2, 1, H, W) and torch.equal(c.grad[:, 0], raw) and bool(raw.any())
    assert g.grad is None and p.grad is None
    _close(raw.cpu().numpy(), _refs(2, H, W), G, "autograd")
    # [B,H,W] in, [B,H,W] gradient out; no policy planes needed
    c3 = _t(cost).requires_grad_(True)
    o3, _ = ops.cost_to_go_tiled(c3, g.detach(), p.detach(), policies=False, differentiable=True)
    assert o3.policies is None and tuple(o3.dists.shape) == (2, 1, H, W)
    (o3.dists[fin] * w[fin]).sum().backward()
    assert tuple(c3.grad.shape) == (2, H, W) and torch.equal(c3.grad, raw)
    # nothing requires a gradient, or grad mode off: detached outputs
    assert not ops.cost_to_go_tiled(c.detach(), g.detach(), p.detach(), differentiable=True)[0].dists.requires_grad
    with torch.no_grad():
        assert not ops.cost_to_go_tiled(c, g, p, differentiable=True)[0].dists.requires_grad


def test_ops_raises_on_a_plateau_and_refuses_capture():
    from neural_astar import ops
    cost, goal, passable, G = _status_batch()
    c, g, p, w = (_t(a)[:, None] for a in (cost, goal, passable, G))
    c.requires_grad_(True)
    with pytest.raises(ValueError, match=r"map\(s\) \[2\] \(1 of 4\)"):
        ops.cost_to_go_tiled(c, g, p, differentiable=True)
    with pytest.raises(ValueError, match=r"map\(s\) \[2\]"):
        ops.cost_to_go_tiled(c.detach(), g, p, differentiable=True)   # the same verdict when nothing asks for a gradient
    assert ops.cost_to_go_tiled(c, g, p)[0].status.tolist() == [0, 3, 0, 0]   # the evaluation call does not mind
    ok = c.detach()[:1].clone().requires_grad_(True)
    want, _ = ops.cost_to_go_tiled(ok, g[:1], p[:1], differentiable=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        marker = g + 1.0                                              # something the capture does hold
        with pytest.raises(RuntimeError, match="cannot be captured"):
            ops.cost_to_go_tiled(ok, g[:1], p[:1], differentiable=True)
        with pytest.raises(RuntimeError, match="cannot be captured"):
            ops.fields_backward_tiled(want.dists.detach(), g[:1], p[:1], w[:1])
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(marker, g + 1.0)
    again, _ = ops.cost_to_go_tiled(ok, g[:1], p[:1], differentiable=True)    # and the call works as before afterwards
    assert again.dists.requires_grad and torch.equal(again.dists, want.dists)


# ---- stream discipline -----------------------------------------------------------------------------------------------------------------------------------------
def test_non_default_stream_with_inputs_produced_on_it():
    from neural_astar import ops
    cost, goal, passable, G = _maps(2, 70, 130)
    fo = _field(cost, goal, passable)
    g, p, base = _t(goal), _t(passable), _t(G)
    want, _, _ = ops.fields_backward_tiled(fo.dists, g, p, base)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=_dev())
    with torch.cuda.stream(side):
        filler = torch.randn(2048, 2048, device=_dev())
        for _ in range(8):                       # work queued ahead of the inputs on the same stream
            filler = filler @ filler * 1e-3
        up = base * 2.0 - base                   # == base bit for bit, produced on `side` behind the filler
        d = fo.dists + 0.0
        got, st, _ = ops.fields_backward_tiled(d, g, p, up)   # every launch, copy and wait of the call is on `side`
    side.synchronize()
    assert st.tolist() == [0, 0] and torch.equal(got, want)


# ---- the planners: value-function supervision reaches the encoder above 128x128's cell count ---------------------------------------------------------------------
def test_neural_astar_trains_its_encoder_against_a_tiled_field():
    from neural_astar import ops
    from neural_astar.planner import NeuralAstar, VanillaAstar
    from neural_astar.planner.differentiable_astar import DifferentiableAstar
    H, W = 80, 96
    rng = np.random.default_rng(80)
    m = (rng.random((2, 1, H, W)) > 0.2).astype(f32)
    s, g = np.zeros_like(m), np.zeros_like(m)
    m[:, 0, 3, 4] = m[:, 0, 70, 90] = 1
    s[:, 0, 3, 4] = g[:, 0, 70, 90] = 1
    m, s, g = _t(m), _t(s), _t(g)
    torch.manual_seed(0)
    na = NeuralAstar(encoder_arch="CNN").to(_dev()).train()
    va = VanillaAstar().to(_dev())
    target = va.cost_to_go_tiled(m, g, policies=False).dists
    out = na.cost_to_go_tiled(m, s, g, differentiable=True)
    assert out.dists.requires_grad and out.policies is not None and not out.policies.requires_grad
    mask = torch.isfinite(out.dists) & torch.isfinite(target)
    assert int(mask.sum()) > 1000
    (out.dists[mask] - target[mask]).abs().mean().backward()
    grads = [q.grad for q in na.encoder.parameters()]
    assert grads and all(x is not None and bool(torch.isfinite(x).all()) for x in grads) and any(bool(x.any()) for x in grads)
    assert not na.cost_to_go_tiled(m, s, g).dists.requires_grad               # the default call is detached
    # the three planners' methods return what ops.cost_to_go_tiled returns
    want, _ = ops.cost_to_go_tiled(m, g, m)
    for got in (va.cost_to_go_tiled(m, g), DifferentiableAstar().cost_to_go_tiled(m, g, m), va.cost_to_go(m, g, tiled=True)):
        assert torch.equal(got.dists, want.dists) and torch.equal(got.policies, want.policies) and torch.equal(got.status, want.status)
    na.eval()
    with torch.no_grad():
        cost = na.encode(m, s, g)
        a = na.cost_to_go_tiled(m, s, g, policies=False)
    b, _ = ops.cost_to_go_tiled(cost, g, m, policies=False)
    assert a.policies is None and torch.equal(a.dists, b.dists)
