"""GPU: the tiled entropy-regularised cost-to-go field and its checkpointed gradient (include/nastar_soft_fields_tiled.h,
``ops.soft_cost_to_go_tiled``).  Where the one-workgroup kernels of include/nastar_soft_fields.h take the map, the tiled calls must give
THEIR bits (``torch.equal``); above their limits the results are held to the float64 definition of tests/soft_fields_oracle.py with the
bounds of that file (``SO.FWD_RTOL`` / ``SO.BWD_RTOL``; the figures are printed before they are asserted).  Every map has 25 % obstacles
and costs U(0.1, 1) unless a case says otherwise.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import soft_fields_oracle as SO
import soft_fields_tiled_cases as TC
from test_soft_fields_gpu import _check_backward, _check_forward, _dev, _t

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
MOORE8 = SO.MOORE8


@functools.lru_cache(maxsize=None)
def _tile():
    from neural_astar import _native
    th, tw, S = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    assert _native.load().nastar_soft_fields_tile(ctypes.addressof(th), ctypes.addressof(tw), ctypes.addressof(S)) == 0
    return th.value, tw.value, S.value


def _seam_shapes():
    """(H, W, B, seed): seams both ways with ragged last tiles; a tile with neighbours above and below"""
    th, tw, _ = _tile()
    return ((th + 3, tw + 5, 2, 12), (2 * th + 1, tw + 1, 1, 13))


def _horizons(H, W):
    S = _tile()[2]
    return sorted({1, S, S + 1, 2 * (H + W)} | ({S - 1} if S > 1 else set()))


def _bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _planted_upstream(seed, live):
    """a random upstream gradient with NaN and +-inf planted on the cells that are not live at the horizon"""
    rng = np.random.default_rng(seed)
    G = rng.standard_normal(live.shape)
    junk = rng.choice(np.array([np.nan, np.inf, -np.inf]), size=live.shape)
    return np.where(live, G, junk)


def _live_at_horizon(dists, passable, goal):
    return (passable != 0) & (goal == 0) & np.isfinite(dists[:, 0].cpu().numpy())


# ---- 1, 2: the bits of the one-workgroup kernels -------------------------------------------------------------------------------------------------------
def _all_shapes():
    return tuple(SO.SHAPE_CASES) + _seam_shapes()


@pytest.mark.parametrize("case", range(len(SO.SHAPE_CASES) + 2))
def test_forward_gives_the_bits_of_the_one_workgroup_kernel(case):
    from neural_astar import ops
    H, W, B, seed = _all_shapes()[case]
    assert H * W <= ops.SOFT_FIELDS_MAX_CELLS
    cost, passable, goal = (_t(a) for a in TC.maps(H, W, B, seed))
    for mask in SO.MASKS:
        for tau in SO.TAUS:
            for K in _horizons(H, W):
                what = f"{B}x{H}x{W} K={K} tau={tau} mask={mask:#05x}"
                ref, _ = ops.soft_fields_forward(cost, goal, passable, tau, K, mask, policies=True)
                out, tape = ops.soft_fields_tiled_forward(cost, goal, passable, tau, K, mask, policies=True)
                assert tape is None and tuple(out.dists.shape) == (B, 1, H, W) and tuple(out.policies.shape) == (B, 8, H, W), what
                assert _bits(out.dists, ref.dists) and _bits(out.policies, ref.policies) and _bits(out.status, ref.status), what
                # ... with a tape too, and without the policy
                out, tape = ops.soft_fields_tiled_forward(cost, goal, passable, tau, K, mask, tape=True, checkpoint_every=3)
                assert out.policies is None and tape is not None and _bits(out.dists, ref.dists) and _bits(out.status, ref.status), what


@pytest.mark.parametrize("case", range(len(SO.SHAPE_CASES) + 1))
def test_backward_gives_the_bits_of_the_one_workgroup_kernel(case):
    from neural_astar import ops
    H, W, B, seed = _all_shapes()[case]
    assert H * W <= ops.SOFT_FIELDS_GRAD_MAX_CELLS
    S = _tile()[2]
    cost_np, passable_np, goal_np = TC.maps(H, W, B, seed)
    cost, passable, goal = (_t(a) for a in (cost_np, passable_np, goal_np))
    moved = 0
    for mask in SO.MASKS:
        for tau in SO.TAUS:
            for K in sorted({1, 2, S + 1, 2 * (H + W)}):
                ref_out, ref_tape = ops.soft_fields_forward(cost, goal, passable, tau, K, mask, tape=True)
                G = _t(_planted_upstream(seed + K, _live_at_horizon(ref_out.dists, passable_np, goal_np)))
                ref, ref_st = ops.soft_fields_backward(cost, goal, passable, ref_tape, G, tau, K, mask)
                assert bool(torch.isfinite(ref).all())
                moved += int(ref.any())
                for c in (1, None, 7, K, K + 5):
                    what = f"{B}x{H}x{W} K={K} tau={tau} mask={mask:#05x} c={c}"
                    out, tape = ops.soft_fields_tiled_forward(cost, goal, passable, tau, K, mask, tape=True, checkpoint_every=c)
                    assert _bits(out.dists, ref_out.dists), what
                    grad, st = ops.soft_fields_tiled_backward(cost, goal, passable, tape, G, tau, K, mask, checkpoint_every=c)
                    assert tuple(grad.shape) == (B, H, W) and _bits(grad, ref) and _bits(st, ref_st), what
    assert moved or H * W == 1


# ---- 3: the result does not depend on the shape of the launches -------------------------------------------------------------------------------------
def test_result_is_independent_of_sweeps_per_launch_and_checkpoint_spacing():
    from neural_astar import ops
    H, W, B, seed, K = TC.ABOVE[1]
    tau = 0.1
    cost_np, passable_np, goal_np = TC.maps(H, W, B, seed)
    cost, passable, goal = (_t(a) for a in (cost_np, passable_np, goal_np))
    out, _ = ops.soft_fields_tiled_forward(cost, goal, passable, tau, K, policies=True)
    one, _ = ops.soft_fields_tiled_forward(cost, goal, passable, tau, K, policies=True, sweeps_per_launch=1)
    again, _ = ops.soft_fields_tiled_forward(cost, goal, passable, tau, K, policies=True)
    for other in (one, again):
        assert _bits(other.dists, out.dists) and _bits(other.policies, out.policies) and _bits(other.status, out.status)
    assert bool(torch.isfinite(out.dists).any()) and bool(out.policies.any())
    G = _t(_planted_upstream(3, _live_at_horizon(out.dists, passable_np, goal_np)))
    grads = []
    for c in (1, None, 10, None):                                   # (None twice: two identical calls)
        o, tape = ops.soft_fields_tiled_forward(cost, goal, passable, tau, K, tape=True, checkpoint_every=c)
        assert _bits(o.dists, out.dists)
        grads.append(ops.soft_fields_tiled_backward(cost, goal, passable, tape, G, tau, K, checkpoint_every=c)[0])
    o, tape = ops.soft_fields_tiled_forward(cost, goal, passable, tau, K, tape=True, checkpoint_every=10, sweeps_per_launch=1)
    grads.append(ops.soft_fields_tiled_backward(cost, goal, passable, tape, G, tau, K, checkpoint_every=10)[0])
    assert bool(grads[0].any()) and bool(torch.isfinite(grads[0]).all())
    for g in grads[1:]:
        assert _bits(g, grads[0])


# ---- 4: above the old limits, against the definition -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,B,seed,K", TC.ABOVE, ids=lambda v: str(v))
def test_field_policy_and_gradient_above_the_old_limits_are_the_definition(H, W, B, seed, K):
    from neural_astar import ops
    assert H * W > ops.SOFT_FIELDS_GRAD_MAX_CELLS
    cost, passable, goal = TC.maps(H, W, B, seed)
    for mask in TC.ABOVE_MASKS:
        for tau in SO.TAUS:
            what = f"{B}x{H}x{W} K={K} tau={tau} mask={mask:#05x}"
            c = _t(cost).requires_grad_(True)
            out = ops.soft_cost_to_go_tiled(c, _t(goal), _t(passable), tau, K, neighbor_mask=mask, policies=True, differentiable=True)
            assert out.dists.requires_grad and not out.policies.requires_grad and tuple(out.dists.shape) == (B, 1, H, W)
            ref_d = _check_forward(out, cost, passable, goal, tau, K, mask, what)   # infinities in place; policy rows; zeros elsewhere
            live = (passable != 0) & (goal == 0) & np.isfinite(ref_d)
            assert live.sum() > 100
            G = TC.upstream(seed, live)
            out.dists.backward(_t(G)[:, None])
            assert tuple(c.grad.shape) == (B, H, W)
            _check_backward(c.grad, cost, passable, goal, G, tau, K, mask, what)    # exactly 0 where the oracle's `ever` is false


# ---- 5: the far corner of the index range ----------------------------------------------------------------------------------------------------------------
def test_far_corner_of_the_largest_map():
    from neural_astar import _native, ops
    H, W, K, tau = TC.CORNER_H, TC.CORNER_W, TC.CORNER_K, TC.CORNER_TAU
    assert H * W == ops.SOFT_FIELDS_TILED_MAX_CELLS == _native.load().nastar_soft_fields_tiled_max_cells()
    cost, passable, goal = TC.corner_maps()
    win = (slice(None),) + TC.CORNER_WINDOW
    c = _t(cost).requires_grad_(True)
    out = ops.soft_cost_to_go_tiled(c, _t(goal), _t(passable), tau, K, policies=True, differentiable=True, checkpoint_every=TC.CORNER_C)
    assert out.status.tolist() == [0]
    d, p = out.dists.detach()[:, 0], out.policies
    # outside the window: +inf and no policy, except nothing -- the goal and everything within K moves of it lie inside
    outside = torch.ones((1, H, W), dtype=torch.bool, device=_dev())
    outside[win] = False
    assert bool(torch.isinf(d[outside]).all()) and bool((d[outside] > 0).all()) and not bool(p[outside[:, None].expand_as(p)].any())
    inner = ops.SoftFieldOutput(out.dists.detach()[:, :, TC.CORNER_WINDOW[0], TC.CORNER_WINDOW[1]],
                                p[:, :, TC.CORNER_WINDOW[0], TC.CORNER_WINDOW[1]], out.status)
    wc, wp, wg = (TC.corner_window(a) for a in (cost, passable, goal))
    ref_d = _check_forward(inner, wc, wp, wg, tau, K, MOORE8, "far corner")
    assert np.isfinite(ref_d).sum() > 20
    G = TC.corner_upstream()
    out.dists.backward(_t(G)[:, None])
    g = c.grad
    assert not bool(g[outside].any()) and not bool(torch.signbit(g[outside]).any())
    ref = _check_backward(g[win], wc, wp, wg, TC.corner_window(G), tau, K, MOORE8, "far corner")
    assert ref[0][TC.CORNER_START[0] - TC.CORNER_WINDOW[0].start, TC.CORNER_START[1] - TC.CORNER_WINDOW[1].start] >= 1
    # one column more is refused
    wide = torch.ones(1, H, W + 1, device=_dev())
    with pytest.raises(NotImplementedError, match="1179648"):
        ops.soft_cost_to_go_tiled(wide, wide, wide, tau, K)
    lib = _native.load()
    ws = torch.empty(lib.nastar_soft_fields_tiled_workspace_bytes(1, H, W + 1), dtype=torch.uint8, device=_dev())
    st = torch.empty(1, dtype=torch.int32, device=_dev())
    rc = lib.nastar_soft_cost_to_go_tiled(wide.data_ptr(), wide.data_ptr(), wide.data_ptr(), 1, H, W + 1, MOORE8, tau, K, torch.empty_like(wide).data_ptr(),
                                          None, st.data_ptr(), None, 0, 1, ws.data_ptr(), ws.numel(), torch.cuda.current_stream(_dev()).cuda_stream)
    assert rc == _native.NASTAR_ERR_UNSUPPORTED


# ---- 6: statuses -------------------------------------------------------------------------------------------------------------------------------------------
def _status_maps():
    (H, W, _, _), _ = _seam_shapes()
    cost, passable, goal = (a.copy() for a in TC.maps(H, W, 7, 23))
    cost[1][tuple(np.argwhere(passable[1] != 0)[5])] = np.nan       # 1: a NaN cost on a passable cell AND no goal: 9 comes first
    goal[1] = 0
    cost[2][tuple(np.argwhere(passable[2] == 0)[0])] = np.nan       # 2: good (an obstacle's cost is not looked at)
    cost[3][tuple(np.argwhere(passable[3] != 0)[-7])] = -0.25       # 3: a negative cost, in the last tile
    goal[4] = 0                                                     # 4: no goal
    goal[5] = 0                                                     # 5: the only goal sits on an obstacle
    goal[5][tuple(np.argwhere(passable[5] == 0)[40])] = 1
    passable[6] = 0                                                 # 6: all obstacles (its goal too)
    return cost, passable, goal, [0, 9, 0, 9, 3, 0, 0]


@pytest.mark.parametrize("tau", SO.TAUS)
def test_statuses_and_the_other_maps_are_unaffected(tau):
    from neural_astar import ops
    cost, passable, goal, want = _status_maps()
    B, H, W = cost.shape
    K = 2 * (H + W)
    tc, tg, tp = _t(cost), _t(goal), _t(passable)
    out, tape = ops.soft_fields_tiled_forward(tc, tg, tp, tau, K, policies=True, tape=True)
    assert out.status.tolist() == want
    good = [0, 2]
    assert all(bool(torch.isfinite(out.dists[b]).sum() > 100) and bool(out.policies[b].any()) for b in good)
    for b in (1, 3, 4, 6):                                          # all +inf, no policy (6: but for its goal cell)
        assert bool(torch.isinf(out.dists[b][tg[b][None] == 0]).all()) and not bool(out.policies[b].any())
    assert bool(torch.isinf(out.dists[1]).all()) and bool(torch.isinf(out.dists[3]).all())
    assert bool((out.dists[5][tg[5][None] != 0] == 0).all()) and bool(torch.isinf(out.dists[5][tg[5][None] == 0]).all())
    G = np.random.default_rng(3).standard_normal(cost.shape)
    grad, st = ops.soft_fields_tiled_backward(tc, tg, tp, tape, _t(G), tau, K)
    assert st.tolist() == [9 if s == 9 else 0 for s in want]
    for b in (1, 3, 4, 5, 6):
        assert not bool(grad[b].any()) and not bool(torch.signbit(grad[b]).any())
    # the bits of the one-workgroup kernels, map by map ...
    ref, ref_tape = ops.soft_fields_forward(tc, tg, tp, tau, K, policies=True, tape=True)
    ref_grad, ref_st = ops.soft_fields_backward(tc, tg, tp, ref_tape, _t(G), tau, K)
    assert _bits(out.dists, ref.dists) and _bits(out.policies, ref.policies) and _bits(out.status, ref.status)
    assert _bits(grad, ref_grad) and _bits(st, ref_st)
    # ... and the good maps alone give the bits they have in this batch
    alone, tape2 = ops.soft_fields_tiled_forward(tc[good], tg[good], tp[good], tau, K, policies=True, tape=True)
    grad2, _ = ops.soft_fields_tiled_backward(tc[good], tg[good], tp[good], tape2, _t(G)[good], tau, K)
    assert _bits(alone.dists, out.dists[good]) and _bits(alone.policies, out.policies[good]) and _bits(grad2, grad[good])
    assert bool(grad2[0].any()) and bool(grad2[1].any())
    with pytest.raises(ValueError, match=r"map\(s\) \[1, 3\]"):
        ops.soft_cost_to_go_tiled(tc, tg, tp, tau, K)


# ---- 7, 8: the maximum-entropy loss on the tiled node ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", TC.MAXENT_TAUS)
def test_maxent_path_nll_tiled_and_its_gradient(tau):
    from neural_astar.planner.differentiable_astar import DifferentiableAstar
    H, W, _, _, K = TC.ABOVE[1]
    B = 2
    cost, passable, goal, start = TC.maxent_maps()                  # 40 moves at least; the optimal route is held below K further down
    planner = DifferentiableAstar().to(_dev())
    demo = planner.shortest_paths_tiled(_t(cost), _t(start), _t(goal), _t(passable))
    assert demo.status.tolist() == [0] * B
    traj = demo.paths.reshape(B, H, W).cpu().numpy().astype(f64)
    assert (traj.sum((1, 2)) - 1 <= K).all() and (traj.sum((1, 2)) - 1 >= 40).all()   # a route among those the partition function counts
    c = _t(cost)[:, None].requires_grad_(True)
    nll = planner.maxent_path_nll(c, _t(start)[:, None], _t(goal)[:, None], _t(passable)[:, None], demo.paths, tau, K, tiled=True)
    assert tuple(nll.shape) == (B,) and nll.requires_grad
    leaves = traj * (goal == 0)
    paid = (cost.astype(f64) * leaves).sum((1, 2))
    V = SO.soft_fields(cost, goal, passable, tau, K)[0]
    ref = (paid - np.where(start != 0, V, 0.0).sum((1, 2))) / tau
    tol = SO.FWD_RTOL * np.abs(V[np.isfinite(V)]).max() / tau
    got = nll.detach().cpu().numpy().astype(f64)
    print(f"tau {tau}: nll {got}, against the definition {np.abs(got - ref).max():.3e} (tol {tol:.3e})")
    assert np.abs(got - ref).max() <= tol and (got >= 0).all()
    nll.sum().backward()
    visits = SO.soft_field_grads(cost, goal, passable, (start != 0).astype(f64), tau, K)[0]
    want = (leaves - visits) / tau
    err = np.abs(c.grad[:, 0].cpu().numpy() - want).max() / (np.abs(visits).max() / tau)
    print(f"tau {tau}: gradient rel err {err:.3e}")
    assert err <= SO.BWD_RTOL
    # the same value and gradient whatever the spacing of the checkpoints
    c2 = _t(cost)[:, None].requires_grad_(True)
    nll2 = planner.maxent_path_nll(c2, _t(start)[:, None], _t(goal)[:, None], _t(passable)[:, None], demo.paths, tau, K, tiled=True, checkpoint_every=1)
    nll2.sum().backward()
    assert _bits(nll2.detach(), nll.detach()) and _bits(c2.grad, c.grad)


def test_neural_astar_trains_its_encoder_on_the_tiled_maxent_loss():
    from neural_astar import ops
    from neural_astar.planner import NeuralAstar, VanillaAstar
    from neural_astar.utils import synthetic as syn
    H, W = 96, 136
    assert H * W == 13056 > ops.SOFT_FIELDS_MAX_CELLS
    Pr = syn.random_obstacle_maps(2, H, W, 0.25, seed=92)
    m, s, g = (_t(a) for a in Pr)
    demo = VanillaAstar().to(_dev()).shortest_paths_tiled(m, s, g)
    assert demo.status.tolist() == [0, 0]
    torch.manual_seed(0)
    na = NeuralAstar(encoder_arch="CNN").to(_dev()).train()
    nll = na.maxent_path_nll(m, s, g, demo.paths, 0.25, tiled=True)
    assert tuple(nll.shape) == (2,) and bool(torch.isfinite(nll).all())
    nll.mean().backward()
    grads = [q.grad for q in na.encoder.parameters()]
    assert grads and all(x is not None and bool(torch.isfinite(x).all()) for x in grads) and any(bool(x.any()) for x in grads)
    with pytest.raises(NotImplementedError, match="6144"):
        na.maxent_path_nll(m, s, g, demo.paths, 0.25, tiled=False)
    out = na.soft_cost_to_go_tiled(m, s, g, 0.25, policies=True)    # differentiable=False: no graph
    assert not out.dists.requires_grad and out.dists.grad_fn is None and not out.policies.requires_grad
