"""GPU: the entropy-regularised cost-to-go field over a finite horizon, its soft policy and its gradient (include/nastar_soft_fields.h,
``ops.soft_cost_to_go``, ``ops.maxent_path_nll``) against the float64 definition of tests/soft_fields_oracle.py -- never against the kernels'
own output.  Every map has 25 % obstacles and costs U(0.1, 1) unless a case says otherwise.  Where the infinities lie must match exactly;
finite values are held to ``SO.FWD_RTOL`` / ``SO.BWD_RTOL`` of the case's scale (the figures are printed before they are asserted).
"""
import functools
import math

import numpy as np
import pytest
import torch

import soft_fields_oracle as SO

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
MOORE8 = SO.MOORE8


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, f32)).to(_dev())


@functools.lru_cache(maxsize=None)
def _maps(H, W, B, seed):
    return SO.random_maps(seed, B, H, W)


def _upstream(seed, live):
    """a random upstream gradient with a NaN on every cell that is not live at the horizon"""
    G = np.random.default_rng(seed).standard_normal(live.shape)
    return np.where(live, G, np.nan)


def _check_forward(out, cost, passable, goal, tau, K, mask, what):
    ref_d, ref_p, ref_st = SO.soft_fields(cost, goal, passable, tau, K, mask)
    d = out.dists.detach()[:, 0].cpu().numpy()
    assert out.status.tolist() == ref_st.tolist(), what
    assert np.array_equal(np.isfinite(d), np.isfinite(ref_d)) and not np.isnan(d).any(), what   # where the infinities lie: exactly
    assert (d[np.isinf(d)] > 0).all() and not d[ref_st != SO.STATUS_BAD_COST][goal[ref_st != SO.STATUS_BAD_COST] != 0].any(), what
    err = SO.rel_err(d, ref_d)
    print(f"{what}: forward rel err {err:.3e}")
    assert err <= SO.FWD_RTOL, what
    if out.policies is not None:
        p = out.policies.cpu().numpy()
        live = (passable != 0) & (goal == 0) & np.isfinite(ref_d)
        rows = p.sum(1)
        assert not p[np.broadcast_to(~live[:, None], p.shape)].any(), what                       # zeros elsewhere, exactly
        if live.any():
            scale = np.abs(ref_d[np.isfinite(ref_d)]).max()
            # pi = softmax(-V_{K-1} / tau): an error dV in a plane moves a probability by at most 2 |dV| / tau of itself; eight terms and a
            # division of one ulp each on top
            tol = 2 * SO.FWD_RTOL * scale / tau + 16 * 2.0 ** -24
            print(f"{what}: policy rows {np.abs(rows[live] - 1).max():.3e}, against the definition {np.abs(p - ref_p).max():.3e} (tol {tol:.3e})")
            assert np.abs(rows[live] - 1).max() <= 16 * 2.0 ** -24 and np.abs(p - ref_p).max() <= tol, what
    return ref_d


def _check_backward(grad, cost, passable, goal, G, tau, K, mask, what):
    ref, ever, _ = SO.soft_field_grads(cost, goal, passable, G, tau, K, mask)
    g = grad.cpu().numpy()
    assert not np.isnan(g).any() and np.isfinite(g).all(), what
    never = g[~ever]
    assert not never.any() and not np.signbit(never).any(), what                                 # +0.0f, bit for bit
    err = SO.rel_err(g, ref)
    print(f"{what}: backward rel err {err:.3e}")
    assert err <= SO.BWD_RTOL, what
    return ref


# ---- the shapes, horizons, temperatures and move sets where the kernels can go wrong ----------------------------------------------------------
@pytest.mark.parametrize("H,W,B,seed", SO.SHAPE_CASES, ids=lambda v: str(v))
def test_field_policy_and_gradient_are_the_definition(H, W, B, seed):
    from neural_astar import ops
    cost, passable, goal = _maps(H, W, B, seed)
    for K, tau, mask in SO.sweep_cases(goal[0], passable[0]):
        what = f"{B}x{H}x{W} K={K} tau={tau} mask={mask:#05x}"
        c = _t(cost).requires_grad_(True)
        out = ops.soft_cost_to_go(c, _t(goal), _t(passable), tau, K, neighbor_mask=mask, policies=True, differentiable=True)
        assert out.dists.requires_grad and not out.policies.requires_grad and tuple(out.dists.shape) == (B, 1, H, W)
        ref_d = _check_forward(out, cost, passable, goal, tau, K, mask, what)
        far = SO.hops(goal[0], passable[0], mask)
        if K == far.max() - 1:                                     # one short: the farthest cell is +inf, the ring before it finite
            d0 = out.dists[0, 0].detach().cpu().numpy()
            assert np.isinf(d0[far == far.max()]).all() and np.isfinite(d0[far == K]).all(), what
        live = (passable != 0) & (goal == 0) & np.isfinite(ref_d)
        G = _upstream(seed, live)
        out.dists.backward(_t(G)[:, None])
        assert tuple(c.grad.shape) == (B, H, W)
        _check_backward(c.grad, cost, passable, goal, G, tau, K, mask, what)


def test_default_horizon_and_the_evaluation_call_builds_no_graph():
    from neural_astar import ops
    H, W = 9, 11
    cost, passable, goal = _maps(H, W, 2, 21)
    c = _t(cost)[:, None].requires_grad_(True)
    out = ops.soft_cost_to_go(c, _t(goal)[:, None], _t(passable)[:, None], 0.5)
    assert out.policies is None and not out.dists.requires_grad and out.dists.grad_fn is None
    _check_forward(out, cost, passable, goal, 0.5, 2 * (H + W), MOORE8, "default horizon")
    with torch.no_grad():
        assert not ops.soft_cost_to_go(c, _t(goal), _t(passable), 0.5, differentiable=True).dists.requires_grad
    assert not ops.soft_cost_to_go(c.detach(), _t(goal), _t(passable), 0.5, differentiable=True).dists.requires_grad
    # [B,1,H,W] in, [B,1,H,W] gradient out
    d = ops.soft_cost_to_go(c, _t(goal), _t(passable), 0.5, differentiable=True).dists
    d[torch.isfinite(d)].sum().backward()
    assert tuple(c.grad.shape) == (2, 1, H, W) and bool(c.grad.any())


# ---- the limits ---------------------------------------------------------------------------------------------------------------------------------
def test_forward_limit_exactly_and_one_cell_more_is_refused():
    from neural_astar import _native, ops
    H, W = 96, 128
    assert H * W == ops.SOFT_FIELDS_MAX_CELLS == _native.load().nastar_soft_fields_max_cells()
    cost, passable, goal = _maps(H, W, 2, 31)
    for K, tau in ((40, 1.0), (2 * (H + W), 0.02)):
        out, tape = ops.soft_fields_forward(_t(cost), _t(goal), _t(passable), tau, K, policies=True)
        assert tape is None
        _check_forward(out, cost, passable, goal, tau, K, MOORE8, f"forward limit K={K} tau={tau}")
    one = torch.ones(1, 1, ops.SOFT_FIELDS_MAX_CELLS + 1, device=_dev())
    with pytest.raises(NotImplementedError, match="12288"):
        ops.soft_cost_to_go(one, one, one, 0.5)
    d = torch.empty_like(one)
    st = torch.empty(1, dtype=torch.int32, device=_dev())
    rc = _native.load().nastar_soft_cost_to_go(one.data_ptr(), one.data_ptr(), one.data_ptr(), 1, 1, ops.SOFT_FIELDS_MAX_CELLS + 1, MOORE8, 0.5, 4,
                                               d.data_ptr(), None, st.data_ptr(), None, 0, torch.cuda.current_stream(_dev()).cuda_stream)
    assert rc == _native.NASTAR_ERR_UNSUPPORTED


def test_backward_limit_exactly():
    from neural_astar import _native, ops
    H, W = 64, 96
    assert H * W == ops.SOFT_FIELDS_GRAD_MAX_CELLS == _native.load().nastar_soft_fields_grad_max_cells()
    cost, passable, goal = _maps(H, W, 2, 32)
    K, tau = 2 * (H + W), 0.1
    c = _t(cost).requires_grad_(True)
    out = ops.soft_cost_to_go(c, _t(goal), _t(passable), tau, K, differentiable=True)
    ref_d = _check_forward(out, cost, passable, goal, tau, K, MOORE8, "backward limit")
    G = _upstream(32, (passable != 0) & (goal == 0) & np.isfinite(ref_d))
    out.dists.backward(_t(G)[:, None])
    _check_backward(c.grad, cost, passable, goal, G, tau, K, MOORE8, "backward limit")
    wide = torch.ones(1, 64, 97, device=_dev(), requires_grad=True)
    with pytest.raises(NotImplementedError, match="6144"):
        ops.soft_cost_to_go(wide, wide, wide, 0.5, differentiable=True)


# ---- degenerate maps --------------------------------------------------------------------------------------------------------------------------------
def _degenerate():
    H, W = 7, 9
    cost, passable, goal = (a.copy() for a in _maps(H, W, 5, 41))
    y, x = np.argwhere(passable[0] == 0)[2]
    goal[0, y, x] = 1                                              # 0: two goals, one of them on an obstacle
    goal[1] = 0                                                    # 1: no goal
    cost[2, 3, 1:8] = 0                                            # 2: a zero-cost strip
    passable[2, 3, 1:8] = 1
    return cost, passable, goal                                    # 3 becomes the BAD_COST map between 2 and 4


@pytest.mark.parametrize("tau", SO.TAUS)
def test_degenerate_maps(tau):
    from neural_astar import ops
    cost, passable, goal = _degenerate()
    K = 20
    c = _t(cost).requires_grad_(True)
    out = ops.soft_cost_to_go(c, _t(goal), _t(passable), tau, K, policies=True, differentiable=True)
    assert out.status.tolist() == [0, 3, 0, 0, 0]
    ref_d = _check_forward(out, cost, passable, goal, tau, K, MOORE8, f"degenerate tau={tau}")
    d = out.dists[:, 0].detach().cpu().numpy()
    assert (goal[0] != 0).sum() == 2 and not d[0][goal[0] != 0].any() and np.isinf(d[1]).all() and np.isfinite(d[2, 3, 1:8]).all()
    G = _upstream(7, (passable != 0) & (goal == 0) & np.isfinite(ref_d))
    out.dists.backward(_t(G)[:, None])
    _check_backward(c.grad, cost, passable, goal, G, tau, K, MOORE8, f"degenerate tau={tau}")
    assert not c.grad[1].any() and bool(c.grad[2, 3, 1:8].any())   # no plateau error here: the strip has a gradient


@pytest.mark.parametrize("value", [float("nan"), -0.25])
def test_one_bad_cost_map_between_two_good_ones(value):
    from neural_astar import ops
    cost, passable, goal = _degenerate()
    cost[3][tuple(np.argwhere(passable[3] != 0)[5])] = value
    cost[4][tuple(np.argwhere(passable[4] == 0)[0])] = np.nan      # an obstacle's cost is not looked at
    out, tape = ops.soft_fields_forward(_t(cost), _t(goal), _t(passable), 0.3, 20, policies=True, tape=True)
    assert out.status.tolist() == [0, 3, 0, 9, 0]
    _check_forward(out, cost, passable, goal, 0.3, 20, MOORE8, "bad cost")
    assert bool(torch.isinf(out.dists[3]).all()) and not out.policies[3].any()
    G = np.random.default_rng(3).standard_normal(cost.shape)
    grad, st = ops.soft_fields_backward(_t(cost), _t(goal), _t(passable), tape, _t(G), 0.3, 20)
    assert st.tolist() == [0, 0, 0, 9, 0] and not grad[3].any()
    _check_backward(grad, cost, passable, goal, G, 0.3, 20, MOORE8, "bad cost")
    with pytest.raises(ValueError, match=r"map\(s\) \[3\]"):
        ops.soft_cost_to_go(_t(cost), _t(goal), _t(passable), 0.3, 20)


# ---- against the existing exact field -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", SO.MASKS)
def test_sandwich_against_the_exact_field_kernel(mask):
    from neural_astar import ops
    import fields_grad_oracle as GO
    H, W, tau = 32, 33, 0.02
    cost, passable, goal = _maps(H, W, 3, 51)
    K = 2 * (H + W)
    D = ops.cost_to_go(_t(cost), _t(goal), _t(passable), neighbor_mask=mask, policies=False).dists[:, 0].cpu().numpy().astype(f64)
    V = ops.soft_cost_to_go(_t(cost), _t(goal), _t(passable), tau, K, neighbor_mask=mask).dists[:, 0].cpu().numpy().astype(f64)
    hops = np.stack([r.hops for r in GO.field_grads(cost, goal, passable, np.zeros_like(cost), mask)])   # the moves of the OPTIMAL route
    within = np.isfinite(D) & (hops <= K)
    assert within.sum() > 20 and np.isfinite(V[within]).all() and np.array_equal(V == 0, D == 0)
    assert not np.isfinite(V[~np.isfinite(D)]).any()
    slack = (SO.FWD_RTOL + K * 2.0 ** -23) * D[within].max()        # the soft kernel's bound, and D's own float32 sum of at most K terms
    lo = D - K * tau * math.log(len(SO.offsets(mask)))
    print(f"mask {mask:#05x}: max V - D {np.max(V[within] - D[within]):.3e}, min V - lower bound {np.min(V[within] - lo[within]):.3e}, slack {slack:.3e}")
    assert (V[within] <= D[within] + slack).all() and (V[within] >= lo[within] - slack).all()


# ---- the same bits twice; the expected visits ---------------------------------------------------------------------------------------------------------
def test_two_calls_agree_bit_for_bit_forward_and_backward():
    from neural_astar import ops
    H, W, B, K, tau = 40, 50, 24, 96, 0.1                           # 2000 cells: four wavefronts per map, several maps per CU
    cost, passable, goal = _maps(H, W, B, 61)
    G = _t(np.random.default_rng(0).standard_normal(cost.shape))
    runs = []
    for _ in range(2):
        out, tape = ops.soft_fields_forward(_t(cost), _t(goal), _t(passable), tau, K, policies=True, tape=True)
        grad, _ = ops.soft_fields_backward(_t(cost), _t(goal), _t(passable), tape, G, tau, K)
        runs.append((out.dists, out.policies, tape, grad))
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert bool(runs[0][3].any())


def test_one_hot_upstream_gives_the_expected_visits():
    from neural_astar import ops
    H, W, tau = 17, 19, 0.3
    cost, passable, goal = _maps(H, W, 3, 71)
    K = 2 * (H + W)
    hops = np.stack([SO.hops(goal[b], passable[b]) for b in range(3)])
    G = np.zeros_like(cost)
    starts = []
    for b in range(3):
        y, x = np.argwhere(hops[b] == hops[b].max())[0]            # the farthest cell: the longest demonstration
        G[b, y, x] = 1
        starts.append((y, x))
    c = _t(cost).requires_grad_(True)
    out = ops.soft_cost_to_go(c, _t(goal), _t(passable), tau, K, differentiable=True)
    out.dists.backward(_t(G)[:, None])
    ref = _check_backward(c.grad, cost, passable, goal, G, tau, K, MOORE8, "one-hot")
    v = c.grad.cpu().numpy().astype(f64)
    for b, (y, x) in enumerate(starts):
        # every route from the start leaves it once at least and has hops(start) moves at least: the mass is the expected length
        tol = SO.BWD_RTOL * np.abs(ref[b]).max() * H * W
        assert (v[b] >= 0).all() and v[b, y, x] >= 1 - tol and v[b].sum() >= hops[b, y, x] - tol and hops[b, y, x] >= 4


# ---- the maximum-entropy loss ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", [0.05, 0.5])
def test_maxent_path_nll_and_its_gradient(tau):
    from neural_astar import ops
    from neural_astar.utils import synthetic as syn
    Pr = syn.random_obstacle_maps(4, 20, 23, 0.25, seed=81)
    H, W = Pr.map_designs.shape[-2:]
    cost = (0.1 + 0.9 * np.random.default_rng(8).random((4, H, W))).astype(f32)
    passable, start, goal = Pr.map_designs[:, 0], Pr.start_maps[:, 0], Pr.goal_maps[:, 0]
    K = 2 * (H + W)
    demo = ops.shortest_paths(_t(cost), _t(start), _t(goal), _t(passable))
    assert demo.status.tolist() == [0] * 4
    c = _t(cost)[:, None].requires_grad_(True)
    nll = ops.maxent_path_nll(c, _t(start)[:, None], _t(goal)[:, None], _t(passable)[:, None], demo.paths, tau)
    assert tuple(nll.shape) == (4,) and nll.requires_grad
    traj = demo.paths.reshape(4, H, W).cpu().numpy().astype(f64)
    leaves = traj * (goal == 0)
    paid = (cost.astype(f64) * leaves).sum((1, 2))
    V = SO.soft_fields(cost, goal, passable, tau, K)[0]
    ref = (paid - np.where(start != 0, V, 0.0).sum((1, 2))) / tau
    # the demonstration's cost is a float32 sum of at most K terms; V is held to FWD_RTOL of its scale
    tol = (K * 2.0 ** -23 * paid.max() + SO.FWD_RTOL * np.abs(V[np.isfinite(V)]).max()) / tau
    got = nll.detach().cpu().numpy().astype(f64)
    print(f"tau {tau}: nll {got}, against the definition {np.abs(got - ref).max():.3e} (tol {tol:.3e})")
    assert (got >= -tol).all() and np.abs(got - ref).max() <= tol
    nll.sum().backward()
    visits = SO.soft_field_grads(cost, goal, passable, (start != 0).astype(f64), tau, K)[0]
    want = (leaves - visits) / tau
    err = np.abs(c.grad[:, 0].cpu().numpy() - want).max() / (np.abs(visits).max() / tau)
    print(f"tau {tau}: gradient rel err {err:.3e}")
    assert err <= SO.BWD_RTOL
    # a start with no goal within the horizon is named
    with pytest.raises(ValueError, match=r"map\(s\) \["):
        ops.maxent_path_nll(c, _t(start), _t(goal), _t(passable), demo.paths, tau, horizon=2)


def test_neural_astar_trains_its_encoder_on_the_maxent_loss():
    from neural_astar.planner import NeuralAstar, VanillaAstar
    from neural_astar.utils import synthetic as syn
    Pr = syn.random_obstacle_maps(2, 32, 32, 0.25, seed=91)
    m, s, g = (_t(a) for a in Pr)
    demo = VanillaAstar().to(_dev()).shortest_paths(m, s, g)
    assert demo.status.tolist() == [0, 0]
    torch.manual_seed(0)
    na = NeuralAstar(encoder_arch="CNN").to(_dev()).train()
    nll = na.maxent_path_nll(m, s, g, demo.paths, 0.25)
    assert tuple(nll.shape) == (2,) and bool(torch.isfinite(nll).all())
    nll.sum().backward()
    grads = [q.grad for q in na.encoder.parameters()]
    assert grads and all(x is not None and bool(torch.isfinite(x).all()) for x in grads) and any(bool(x.any()) for x in grads)
    out = na.soft_cost_to_go(m, s, g, 0.25, policies=True)          # differentiable=False: no graph
    assert not out.dists.requires_grad and out.dists.grad_fn is None and not out.policies.requires_grad
    assert na.soft_cost_to_go(m, s, g, 0.25, differentiable=True).dists.requires_grad
