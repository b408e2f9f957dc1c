"""GPU (-m gpu): the gradient of the cost-to-go field with respect to the cost maps (include/nastar_fields_grad.h, ``ops.fields_backward``,
``ops.cost_to_go(..., differentiable=True)``) against the numpy float64 definition (tests/fields_grad_oracle.py, pinned on the CPU by
tests/test_fields_grad.py).

The tolerance of every comparison with the definition is derived, not tuned: |got - ref| <= 2^-23 |ref| + 1e-9 sum|G| over the live cells of
that map -- one fp32 rounding at the store (2^-24 relative) doubled, and a generous ceiling for what the ORDER of an fp64 accumulation of up
to 16384 signed terms can change (16384 x 2^-53 sum|G| < 2e-12 sum|G|).  Cells that are not live are exactly 0.0.  Costs are U(0.5, 1.5):
at these sizes D < 2^14, ulp(D) <= 2^-9 < 0.5, so no addition is absorbed and no map has a plateau -- asserted on the definition.
"""
import functools

import numpy as np
import pytest
import torch

import fields_grad_oracle as GO
import heuristic_oracle as HO

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
DIRECTED = 0x0EB  # one of the asymmetric move sets of the neighbour tests
SHAPES = [(1, 1), (1, 9), (7, 5), (20, 45), (32, 32), (64, 64)]


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).to(_dev())  # (a copy: the shared inputs are read-only)


@functools.lru_cache(maxsize=None)
def _case(H, W, goals=1, seed=0, goal_on_obstacle=False):
    """3 seeded maps [3,H,W]: cost U(0.5, 1.5), goal (``goals`` cells per map, the first on a passable cell), passable (about 30 % obstacles;
    on a square map of 32 cells a side or more, map 2 is a maze of ``utils.synthetic`` with its own goal), upstream gradient N(0, 1).
    ``goal_on_obstacle``: map 0 gets one more goal, on an obstacle cell.  Shared between tests, never modified."""
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
    if goal_on_obstacle:
        walls = np.argwhere(passable[0] == 0)
        goal[0][tuple(walls[rng.integers(len(walls))])] = 1
    cost = (0.5 + rng.random((B, H, W))).astype(f32)
    G = rng.standard_normal((B, H, W)).astype(f32)
    for a in (cost, goal, passable, G):
        a.setflags(write=False)
    return cost, goal, passable, G


@functools.lru_cache(maxsize=None)
def _ref(H, W, goals=1, seed=0, goal_on_obstacle=False, mask=HO.MOORE8):
    cost, goal, passable, G = _case(H, W, goals, seed, goal_on_obstacle)
    refs = GO.field_grads(cost, goal, passable, G, mask)
    assert all(r.status == 0 for r in refs), "U(0.5, 1.5) costs have no plateau at these sizes"
    return refs


def _forward(cost, goal, passable, mask=None, policies=False):
    from neural_astar import ops
    return ops.cost_to_go(_t(cost)[:, None], _t(goal)[:, None], _t(passable)[:, None], neighbor_mask=mask, policies=policies)


def _backward(dists, goal, passable, G, mask=None, sweeps=False):
    """the raw entry point on device tensors -> (grad_cost [B,H,W] numpy, status list, sweeps list or None)"""
    from neural_astar import ops
    B = dists.shape[0]
    sw = torch.full((B,), -7, dtype=torch.int32, device=_dev()) if sweeps else None
    grad, status = ops.fields_backward(dists, _t(goal), _t(passable), _t(G), neighbor_mask=mask, sweeps_out=sw)
    assert grad.dtype == torch.float32 and tuple(grad.shape) == (B,) + tuple(dists.shape[-2:]) and not grad.requires_grad
    return grad.cpu().numpy(), status.tolist(), (sw.tolist() if sweeps else None)


def _close(got, refs, G, what=""):
    """got [B,H,W] against the definition, at the derived tolerance; exactly 0.0 where not live"""
    worst = 0.0
    for b, r in enumerate(refs):
        assert not got[b][~r.live].any(), f"{what}: map {b} has a non-zero gradient on a cell that is not live"
        tol = 2.0 ** -23 * np.abs(r.A) + 1e-9 * np.abs(G[b][r.live].astype(f64)).sum()
        err = np.abs(got[b].astype(f64) - r.A)
        if r.live.any():
            worst = max(worst, float((err[r.live] / np.maximum(tol[r.live], 1e-300)).max()))
        assert (err[r.live] <= tol[r.live]).all(), f"{what}: map {b}: max err {err[r.live].max():.3e}, {int((err > tol)[r.live].sum())} cells over the tolerance"
    print(f"{what}: worst |got - ref| / tolerance = {worst:.3f}")


def _parity(H, W, mask=HO.MOORE8, goals=1, goal_on_obstacle=False, nan_dead=False, seed=0):
    cost, goal, passable, G = _case(H, W, goals, seed, goal_on_obstacle)
    refs = _ref(H, W, goals, seed, goal_on_obstacle, mask)
    fo = _forward(cost, goal, passable, mask)
    assert np.array_equal(fo.dists[:, 0].cpu().numpy(), np.stack([r.dist for r in refs]))
    if nan_dead:  # whatever arrives for a cell that is not live is never read
        G = np.where(np.stack([r.live for r in refs]), G, f32(np.nan))
    got, status, _ = _backward(fo.dists, goal, passable, G, mask)
    assert status == [0, 0, 0]
    _close(got, refs, G, f"{H}x{W} mask {mask:#x} K={goals}")
    return refs


# ---- the definition: shapes x move sets, goals, what is not live --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", [HO.MOORE8, HO.VON_NEUMANN, DIRECTED])
@pytest.mark.parametrize("H,W", SHAPES)
def test_oracle_parity(H, W, mask):
    refs = _parity(H, W, mask)
    if H * W >= 900 and mask != DIRECTED:  # the case is not a trivial one: trees of some height, cells with several children
        assert max(int(r.hops.max()) for r in refs) > 10
        kids = np.bincount(refs[0].succ[refs[0].live], minlength=H * W)
        assert kids.max() >= 2


@pytest.mark.parametrize("H,W", [(7, 5), (20, 45), (32, 32)])
def test_nearest_of_three_goals_and_a_goal_on_an_obstacle(H, W):
    refs = _parity(H, W, goals=3, goal_on_obstacle=True, seed=1)
    _, goal, passable, _ = _case(H, W, 3, 1, True)
    assert ((goal[0] != 0) & (passable[0] == 0)).any() and (goal != 0).reshape(3, -1).sum(1).max() >= 3
    assert all(not r.live[goal[b] != 0].any() for b, r in enumerate(refs))


@pytest.mark.parametrize("H,W,mask", [(20, 45, HO.MOORE8), (64, 64, HO.VON_NEUMANN)])
def test_gradient_on_cells_that_are_not_live_is_never_read(H, W, mask):
    refs = _parity(H, W, mask, nan_dead=True)
    assert sum(int((~r.live).sum()) for r in refs) > 10


# ---- the largest map: a forest about 8192 edges high ------------------------------------------------------------------------------------------------------
def _serpentine(H, W, flip):
    """rows 0, 2, 4, ... are corridors, the odd rows walls with ONE door, at the right and the left end in turn; 4-connected moves: the
    successor of every cell is forced.  -> (passable [H,W], the corridor as a list of flat indices from the goal on)"""
    passable = np.zeros((H, W), f32)
    path = []
    for r in range(H):
        if r % 2 == 0:
            cols = range(W) if (r // 2) % 2 == 0 else range(W - 1, -1, -1)
        else:
            cols = [W - 1] if (r // 2) % 2 == 0 else [0]
        for c in cols:
            passable[r, c] = 1
            path.append(r * W + c)
    if flip:  # the goal in the last row: the chain runs up the map
        passable = passable[::-1].copy()
        path = [(H - 1 - i // W) * W + i % W for i in path]
    return passable, path


def test_largest_map_subtree_sizes_are_exact():
    H = W = 128
    maps = [_serpentine(H, W, flip) for flip in (False, True)]
    passable = np.stack([m[0] for m in maps])
    goal = np.zeros((2, H, W), f32)
    want = np.zeros((2, H * W), f32)
    for b, (_, path) in enumerate(maps):
        goal[b].reshape(-1)[path[0]] = 1
        want[b][path[1:]] = np.arange(len(path) - 1, 0, -1)   # the cell j moves from the goal carries every cell behind it, and itself
    assert len(maps[0][1]) == 64 * 128 + 64 and want.max() == 8255 < 2 ** 24
    fo = _forward(passable, goal, passable, HO.VON_NEUMANN)   # unit costs: D is the number of moves
    d = fo.dists[:, 0].cpu().numpy().reshape(2, -1)
    for b, (_, path) in enumerate(maps):
        assert np.array_equal(d[b][path], np.arange(len(path), dtype=f32))
    got, status, sweeps = _backward(fo.dists, goal, passable, np.ones((2, H, W), f32), HO.VON_NEUMANN, sweeps=True)
    assert status == [0, 0]
    assert np.array_equal(got.reshape(2, -1), want)
    print(f"128x128 serpentine, forest height {len(maps[0][1]) - 2}: sweeps {sweeps}")
    assert all(2 <= s <= H * W for s in sweeps)


# ---- against a kernel the tree already trusts: the policy roll-out ------------------------------------------------------------------------------------------
def test_one_hot_gradient_is_the_policy_rollout():
    from neural_astar import _native
    from neural_astar.utils import synthetic as syn
    H = W = 32
    P = syn.maze_maps(1, H, seed=21)
    passable, goal = P.map_designs[:, 0], P.goal_maps[:, 0]
    cost = (0.5 + np.random.default_rng(3).random((1, H, W))).astype(f32)
    fo = _forward(cost, goal, passable, policies=True)
    d = fo.dists[0, 0].cpu().numpy()
    live = np.flatnonzero((np.isfinite(d) & (goal[0] == 0)).reshape(-1))
    starts = np.random.default_rng(4).choice(live, 8, replace=False).astype(np.int32)
    G = np.zeros((8, H * W), f32)
    G[np.arange(8), starts] = 1
    rep = lambda a: np.repeat(a, 8, axis=0)  # noqa: E731
    got, status, _ = _backward(fo.dists.expand(8, 1, H, W).contiguous(), rep(goal), rep(passable), G.reshape(8, H, W))
    assert status == [0] * 8
    si, gi = _t(starts.reshape(1, 8)), _t(np.array([goal.reshape(-1).argmax()], np.int32))
    trajs = torch.empty((1, 8, H, W), dtype=torch.float32, device=_dev())
    st = torch.empty((8,), dtype=torch.int32, device=_dev())
    rc = _native.load().nastar_policy_rollout(fo.policies.data_ptr(), si.data_ptr(), gi.data_ptr(), 1, 8, 8, H, W, trajs.data_ptr(), st.data_ptr(),
                                              torch.cuda.current_stream(_dev()).cuda_stream)
    assert rc == 0 and st.tolist() == [0] * 8
    assert np.array_equal(got, trajs[0].cpu().numpy()) and got.sum() >= 8


# ---- the identity that ties the gradient to the field -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(20, 45), (32, 32)])
def test_gradient_times_cost_sums_to_the_field(H, W):
    """G = 1 on live cells: every cell pays its cost once per roll-out through it, so sum(grad_cost * cost) is the sum of D over the live
    cells -- up to the forward's roundings, one per hop: hops_max * 2^-24 relative"""
    cost, goal, passable, _ = _case(H, W)
    refs = _ref(H, W)
    fo = _forward(cost, goal, passable)
    got, status, _ = _backward(fo.dists, goal, passable, np.ones((3, H, W), f32))
    d = fo.dists[:, 0].cpu().numpy()
    assert status == [0, 0, 0]
    for b, r in enumerate(refs):
        lhs = float((got[b].astype(f64) * cost[b].astype(f64)).sum())
        rhs = float(d[b][r.live].astype(f64).sum())
        print(f"{H}x{W} map {b}: sum(grad * cost) = {lhs!r}, sum(D) = {rhs!r}, hops_max {int(r.hops.max())}")
        assert np.array_equal(got[b], np.round(got[b])) and abs(lhs - rhs) <= int(r.hops.max()) * 2.0 ** -24 * rhs


def test_two_calls_give_the_same_bits():
    cost, goal, passable, G = _case(64, 64)
    fo = _forward(cost, goal, passable)
    from neural_astar import ops
    g, p, u = _t(goal), _t(passable), _t(G)
    a, _ = ops.fields_backward(fo.dists, g, p, u)
    b, _ = ops.fields_backward(fo.dists, g, p, u)
    assert torch.equal(a, b) and bool(a.any())


# ---- statuses: four maps, four stories, one launch ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _status_batch():
    """map 0 ordinary; map 1 without a goal; map 2 with a zero-cost strip; map 3 ordinary"""
    cost, goal, passable, G = (np.concatenate([a, a[:1]]) for a in _case(20, 45))
    goal[1] = 0
    y, x = np.argwhere(goal[2] != 0)[0]
    xs = slice(max(0, x - 3), min(45, x + 4))
    passable[2, y, xs] = 1
    cost[2, y, xs] = 0
    cost[3], goal[3], passable[3], G[3] = (a[1] for a in _case(20, 45, seed=5))
    return cost, goal, passable, G


def test_statuses_in_one_batch():
    cost, goal, passable, G = _status_batch()
    refs = GO.field_grads(cost, goal, passable, G)
    assert [r.status for r in refs] == [0, 0, 11, 0] and not refs[1].live.any() and refs[3].live.sum() > 50
    fo = _forward(cost, goal, passable)
    assert fo.status.tolist() == [0, 3, 0, 0]
    got, status, sweeps = _backward(fo.dists, goal, passable, G, sweeps=True)
    assert status == [0, 0, 11, 0] and sweeps[1] == 0 and sweeps[2] == 0 and sweeps[0] >= 1 and sweeps[3] >= 1
    assert not got[1].any() and not got[2].any()
    _close(got[[0, 3]], [refs[0], refs[3]], G[[0, 3]], "statuses")
    alone, st, _ = _backward(fo.dists[3:4], goal[3:4], passable[3:4], G[3:4])   # the others leave no trace in map 3
    assert st == [0] and np.array_equal(alone[0], got[3])


def test_ops_raises_on_a_plateau_and_refuses_tiled_and_capture():
    from neural_astar import ops
    cost, goal, passable, _ = _status_batch()
    c, g, p = (_t(a)[:, None] for a in (cost, goal, passable))
    c.requires_grad_(True)
    with pytest.raises(ValueError, match=r"map\(s\) \[2\] \(1 of 4\)"):
        ops.cost_to_go(c, g, p, differentiable=True)
    with pytest.raises(ValueError, match=r"map\(s\) \[2\]"):
        ops.cost_to_go(c.detach(), g, p, differentiable=True)      # the same verdict when nothing asks for a gradient
    assert ops.cost_to_go(c, g, p).status.tolist() == [0, 3, 0, 0]  # the evaluation call does not mind
    with pytest.raises(NotImplementedError, match="tiled"):
        ops.cost_to_go(c, g, p, tiled=True, differentiable=True)
    ok = c.detach()[:1].clone().requires_grad_(True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        marker = g + 1.0                                            # something the capture does hold
        with pytest.raises(NotImplementedError, match="cannot be captured"):
            ops.cost_to_go(ok, g[:1], p[:1], differentiable=True)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(marker, g + 1.0)
    assert ops.cost_to_go(ok, g[:1], p[:1], differentiable=True).dists.requires_grad   # and the call works as before afterwards


# ---- autograd ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_autograd_is_the_raw_entry_point():
    from neural_astar import ops
    cost, goal, passable, G = _case(20, 45)
    c, g, p, w = (_t(a)[:, None] for a in (cost, goal, passable, G))
    c.requires_grad_(True)
    g.requires_grad_(True)
    p.requires_grad_(True)
    plain = ops.cost_to_go(c, g, p)
    assert not plain.dists.requires_grad and plain.dists.grad_fn is None     # the default is today's call
    out = ops.cost_to_go(c, g, p, differentiable=True)
    assert out.dists.requires_grad and not out.policies.requires_grad and not out.status.requires_grad
    assert torch.equal(out.dists, plain.dists) and torch.equal(out.policies, plain.policies) and torch.equal(out.status, plain.status)
    fin = torch.isfinite(out.dists)
    (out.dists[fin] * w[fin]).sum().backward()
    raw, st = ops.fields_backward(plain.dists, g.detach(), p.detach(), torch.where(fin, w, torch.zeros_like(w)))
    assert st.tolist() == [0, 0, 0]
    assert tuple(c.grad.shape) == (3, 1, 20, 45) and torch.equal(c.grad[:, 0], raw) and bool(raw.any())
    assert g.grad is None and p.grad is None
    _close(raw.cpu().numpy(), _ref(20, 45), G, "autograd")
    # [B,H,W] in, [B,H,W] gradient out; no policy planes needed
    c3 = _t(cost).requires_grad_(True)
    o3 = ops.cost_to_go(c3, g.detach(), p.detach(), policies=False, differentiable=True)
    assert o3.policies is None and tuple(o3.dists.shape) == (3, 1, 20, 45)
    (o3.dists[fin] * w[fin]).sum().backward()
    assert tuple(c3.grad.shape) == (3, 20, 45) and torch.equal(c3.grad, raw)
    with torch.no_grad():                                                     # grad mode off: no node
        assert not ops.cost_to_go(c, g, p, differentiable=True).dists.requires_grad


# ---- the planner: value-function supervision reaches the encoder ---------------------------------------------------------------------------------------------------
def test_neural_astar_trains_its_encoder_against_a_field():
    from neural_astar.planner import NeuralAstar, VanillaAstar
    from neural_astar.utils import synthetic as syn
    P = syn.maze_maps(4, 32, seed=31)
    m, s, g = (_t(a) for a in P)
    torch.manual_seed(0)
    na = NeuralAstar(encoder_arch="CNN").to(_dev()).train()
    target = VanillaAstar().to(_dev()).cost_to_go(m, g, policies=False).dists
    seen = []
    encode = na.encode

    def keeping(*args, **kw):
        cost = encode(*args, **kw)
        cost.retain_grad()
        seen.append(cost)
        return cost

    na.encode = keeping
    out = na.cost_to_go(m, s, g, differentiable=True)
    assert out.dists.requires_grad and len(seen) == 1
    out.dists.retain_grad()
    mask = torch.isfinite(out.dists) & torch.isfinite(target)
    (out.dists[mask] - target[mask]).abs().mean().backward()
    grads = [q.grad for q in na.encoder.parameters()]
    assert grads and all(x is not None and bool(torch.isfinite(x).all()) for x in grads) and any(bool(x.any()) for x in grads)
    cost, G = seen[0].detach().cpu().numpy(), out.dists.grad.cpu().numpy()
    refs = GO.field_grads(cost, P.goal_maps, P.map_designs, G)
    assert all(r.status == 0 for r in refs)
    assert np.array_equal(out.dists.detach()[:, 0].cpu().numpy(), np.stack([r.dist for r in refs]))
    _close(seen[0].grad[:, 0].cpu().numpy(), refs, G[:, 0], "NeuralAstar")
    na.encode = encode
    assert not na.cost_to_go(m, s, g).dists.requires_grad                     # and the default call is the detached one it was
