"""GPU: the log-policy of the tiled entropy-regularised cost-to-go field and the gradient through it (include/nastar_soft_policy_tiled.h,
``ops.soft_policy_tiled``, ``ops.soft_policy_nll_tiled``).  Where the one-workgroup kernels of include/nastar_soft_policy.h take the map, the
tiled calls must give THEIR bits, and the bits of the tiled field calls in what those write; above the one-workgroup limits the results are
held to the float64 definitions of tests/soft_policy_oracle.py and tests/soft_fields_oracle.py: where -inf lies exactly, a finite
log-probability to the bound of tests/test_soft_policy_gpu.py, a gradient to ``PC.PTILED_RTOL`` of the case's max |gradient| (the figures
are printed before they are asserted).  Every map has 25 % obstacles and costs U(0.1, 1) unless a case says otherwise.
"""
import numpy as np
import pytest
import torch

import soft_fields_oracle as SO
import soft_fields_tiled_cases as TC
import soft_policy_oracle as PO
import soft_policy_tiled_cases as PC
from test_soft_fields_gpu import _dev, _t
from test_soft_fields_tiled_gpu import _all_shapes, _bits, _horizons, _planted_upstream, _seam_shapes, _tile
from test_soft_policy_gpu import _check_log_policy

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
MOORE8 = SO.MOORE8
EPS = 2.0 ** -24


def _zero(t):
    """all +0.0f, bit for bit"""
    return not bool(t.any()) and not bool(torch.signbit(t).any())


def _check_grad(grad, ref, ever, what):
    g = grad.cpu().numpy()
    assert np.isfinite(g).all(), what
    never = g[~ever]
    assert not never.any() and not np.signbit(never).any(), what                                 # +0.0f, bit for bit
    err = SO.rel_err(g, ref)
    print(f"{what}: gradient rel err {err:.3e} (bound {PC.PTILED_RTOL:.3e})")
    assert err <= PC.PTILED_RTOL, what


# ---- 1, 2: the bits of the one-workgroup kernels and of the tiled field calls ---------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(SO.SHAPE_CASES) + 2))
def test_forward_gives_the_bits_of_the_one_workgroup_kernel_and_of_the_tiled_field(case):
    from neural_astar import ops
    H, W, B, seed = _all_shapes()[case]
    assert H * W <= ops.SOFT_FIELDS_MAX_CELLS
    cost, passable, goal = (_t(a) for a in TC.maps(H, W, B, seed))
    finite = 0
    for mask in SO.MASKS:
        for tau in SO.TAUS:
            for K in _horizons(H, W):
                what = f"{B}x{H}x{W} K={K} tau={tau} mask={mask:#05x}"
                ref, _ = ops.soft_policy_forward(cost, goal, passable, tau, K, mask, policies=True)
                out, tape = ops.soft_policy_tiled_forward(cost, goal, passable, tau, K, mask, policies=True, tape=True, checkpoint_every=3)
                assert tuple(out.log_policies.shape) == (B, 8, H, W) == tuple(out.policies.shape) and tuple(out.dists.shape) == (B, 1, H, W), what
                assert _bits(out.dists, ref.dists) and _bits(out.log_policies, ref.log_policies) and _bits(out.policies, ref.policies), what
                assert _bits(out.status, ref.status), what
                fld, fld_tape = ops.soft_fields_tiled_forward(cost, goal, passable, tau, K, mask, policies=True, tape=True, checkpoint_every=3)
                assert _bits(out.dists, fld.dists) and _bits(out.policies, fld.policies) and _bits(out.status, fld.status), what
                assert _bits(tape, fld_tape), what
                # without the policy, and without a tape: no other output changes
                nopol, none = ops.soft_policy_tiled_forward(cost, goal, passable, tau, K, mask, policies=False)
                assert nopol.policies is None and none is None, what
                assert _bits(nopol.log_policies, out.log_policies) and _bits(nopol.dists, out.dists) and _bits(nopol.status, out.status), what
                finite += int(torch.isfinite(out.log_policies).any())
    assert finite or H * W == 1


@pytest.mark.parametrize("case", range(len(SO.SHAPE_CASES) + 1))
def test_backward_gives_the_bits_of_the_one_workgroup_kernel_and_of_the_tiled_field(case):
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
                ref_out, ref_tape = ops.soft_policy_forward(cost, goal, passable, tau, K, mask, tape=True)
                # (live at K, Act) is where the one-workgroup log-policy is finite: tests/test_soft_policy_gpu.py holds that to the definition
                act = torch.isfinite(ref_out.log_policies).cpu().numpy()
                G = _t(_planted_upstream(seed + K, act.any(1)))                  # NaN and +-inf off the live cells
                GL = _t(PO.upstream(seed + K, act))                              # NaN outside (live at K, Act)
                ref_alone, ref_st = ops.soft_policy_backward(cost, goal, passable, ref_tape, None, GL, tau, K, mask)
                ref_both, _ = ops.soft_policy_backward(cost, goal, passable, ref_tape, G, GL, tau, K, mask)
                assert bool(torch.isfinite(ref_alone).all()) and bool(torch.isfinite(ref_both).all())
                moved += int(ref_alone.any())
                for c in sorted({1, K, K + 5} | ({K - 1} if K >= 2 else set())) + [None]:   # (K - 1: plane K - 1 is itself a checkpoint)
                    what = f"{B}x{H}x{W} K={K} tau={tau} mask={mask:#05x} c={c}"
                    out, tape = ops.soft_policy_tiled_forward(cost, goal, passable, tau, K, mask, tape=True, checkpoint_every=c)
                    assert _bits(out.log_policies, ref_out.log_policies), what
                    alone, st = ops.soft_policy_tiled_backward(cost, goal, passable, tape, None, GL, tau, K, mask, checkpoint_every=c)
                    assert tuple(alone.shape) == (B, H, W) and _bits(alone, ref_alone) and _bits(st, ref_st), what
                    both, _ = ops.soft_policy_tiled_backward(cost, goal, passable, tape, G, GL, tau, K, mask, checkpoint_every=c)
                    assert _bits(both, ref_both), what
                    field, _ = ops.soft_policy_tiled_backward(cost, goal, passable, tape, G, None, tau, K, mask, checkpoint_every=c)
                    assert _bits(field, ops.soft_fields_tiled_backward(cost, goal, passable, tape, G, tau, K, mask, checkpoint_every=c)[0]), what
                    none, _ = ops.soft_policy_tiled_backward(cost, goal, passable, tape, None, None, tau, K, mask, checkpoint_every=c)
                    assert _zero(none), what
                    if K == 1:
                        assert _zero(alone) and _bits(both, field), what         # GL is not read: exactly 0.0f
                    # either tiled forward's tape
                    _, fld_tape = ops.soft_fields_tiled_forward(cost, goal, passable, tau, K, mask, tape=True, checkpoint_every=c)
                    other, _ = ops.soft_policy_tiled_backward(cost, goal, passable, fld_tape, G, GL, tau, K, mask, checkpoint_every=c)
                    assert _bits(other, ref_both), what
    assert moved or H * W == 1


# ---- 3: the result does not depend on the shape of the launches -------------------------------------------------------------------------------------
def test_result_is_independent_of_sweeps_per_launch_and_checkpoint_spacing():
    from neural_astar import ops
    H, W, B, seed, K = TC.ABOVE[1]
    tau = 0.1
    cost, passable, goal = (_t(a) for a in TC.maps(H, W, B, seed))
    out, _ = ops.soft_policy_tiled_forward(cost, goal, passable, tau, K)
    one, _ = ops.soft_policy_tiled_forward(cost, goal, passable, tau, K, sweeps_per_launch=1)
    again, _ = ops.soft_policy_tiled_forward(cost, goal, passable, tau, K)
    for other in (one, again):
        assert _bits(other.log_policies, out.log_policies) and _bits(other.dists, out.dists) and _bits(other.policies, out.policies)
    act = torch.isfinite(out.log_policies).cpu().numpy()
    assert act.sum() > 1000
    G, GL = _t(_planted_upstream(3, act.any(1))), _t(PO.upstream(4, act))
    grads = []
    for c in (1, None, 10, None):                                   # (None twice: two identical calls)
        o, tape = ops.soft_policy_tiled_forward(cost, goal, passable, tau, K, tape=True, checkpoint_every=c)
        assert _bits(o.log_policies, out.log_policies)
        grads.append(ops.soft_policy_tiled_backward(cost, goal, passable, tape, G, GL, tau, K, checkpoint_every=c)[0])
    o, tape = ops.soft_policy_tiled_forward(cost, goal, passable, tau, K, tape=True, checkpoint_every=10, sweeps_per_launch=1)
    assert _bits(o.log_policies, out.log_policies)
    grads.append(ops.soft_policy_tiled_backward(cost, goal, passable, tape, G, GL, tau, K, checkpoint_every=10)[0])
    assert bool(grads[0].any()) and bool(torch.isfinite(grads[0]).all())
    for g in grads[1:]:
        assert _bits(g, grads[0])
    alone = ops.soft_policy_tiled_backward(cost, goal, passable, tape, None, GL, tau, K, checkpoint_every=10)[0]
    assert bool(alone.any()) and bool(torch.isfinite(alone).all()) and not _bits(alone, grads[0])


# ---- 4: above the old limits, against the definition -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", SO.TAUS)
@pytest.mark.parametrize("mask", TC.ABOVE_MASKS, ids=lambda m: f"{m:#05x}")
@pytest.mark.parametrize("H,W,B,seed,K", TC.ABOVE, ids=lambda v: str(v))
def test_log_policy_and_gradient_above_the_old_limits_are_the_definition(H, W, B, seed, K, mask, tau):
    from neural_astar import ops
    assert H * W > ops.SOFT_FIELDS_GRAD_MAX_CELLS
    cost, passable, goal = TC.maps(H, W, B, seed)
    what = f"{B}x{H}x{W} K={K} tau={tau} mask={mask:#05x}"
    c = _t(cost).requires_grad_(True)
    out = ops.soft_policy_tiled(c, _t(goal), _t(passable), tau, K, neighbor_mask=mask)
    assert out.dists.grad_fn is not None and out.dists.grad_fn is out.log_policies.grad_fn and not out.policies.requires_grad
    assert tuple(out.log_policies.shape) == (B, 8, H, W) and out.status.tolist() == [0] * B
    _, act = _check_log_policy(out, cost, passable, goal, tau, K, mask, what)   # -inf in place; the bound; exp(logpi) against the policy
    assert act.sum() > 500
    G, GL = PC.upstreams(seed, act)
    parts = [PO.soft_policy_grad(cost[b], goal[b], passable[b], G[b], GL[b], tau, K, mask) for b in range(B)]
    ever = np.stack([q.ever for q in parts])
    torch.autograd.backward([out.log_policies], [_t(GL)], retain_graph=True)    # GL alone
    assert tuple(c.grad.shape) == (B, H, W)
    _check_grad(c.grad, np.stack([q.policy_part for q in parts]), ever, what + " GL alone")
    c.grad = None
    torch.autograd.backward([out.dists, out.log_policies], [_t(G)[:, None], _t(GL)])   # ONE node: both seeds in one call
    _check_grad(c.grad, np.stack([q.grad for q in parts]), ever, what + " GL and G")


# ---- 5: the far corner of the index range ----------------------------------------------------------------------------------------------------------------
def test_far_corner_of_the_largest_map():
    from neural_astar import _native, ops
    H, W, K, tau = TC.CORNER_H, TC.CORNER_W, TC.CORNER_K, TC.CORNER_TAU
    assert H * W == ops.SOFT_FIELDS_TILED_MAX_CELLS == _native.load().nastar_soft_fields_tiled_max_cells()
    cost, passable, goal = TC.corner_maps()
    win = (slice(None), slice(None)) + TC.CORNER_WINDOW
    c = _t(cost).requires_grad_(True)
    out = ops.soft_policy_tiled(c, _t(goal), _t(passable), tau, K, checkpoint_every=TC.CORNER_C)
    assert out.status.tolist() == [0]
    lp = out.log_policies.detach()
    outside = torch.ones((1, 8, H, W), dtype=torch.bool, device=_dev())
    outside[win] = False
    assert bool(torch.isneginf(lp[outside]).all())                  # the goal and everything within K moves of it lie inside the window
    inner = ops.SoftPolicyOutput(out.dists.detach()[win], lp[win], out.policies[win], out.status)
    wc, wp, wg = (TC.corner_window(a) for a in (cost, passable, goal))
    _, act = _check_log_policy(inner, wc, wp, wg, tau, K, MOORE8, "far corner")
    sy, sx = TC.CORNER_START[0] - TC.CORNER_WINDOW[0].start, TC.CORNER_START[1] - TC.CORNER_WINDOW[1].start
    assert act.sum() > 20 and act[0, :, sy, sx].sum() >= 2
    a = int(np.argmax(act[0, :, sy, sx]))                           # a one-hot GL on one action of the start
    GL = torch.zeros((1, 8, H, W), dtype=torch.float32, device=_dev())
    GL[0, a, TC.CORNER_START[0], TC.CORNER_START[1]] = 1
    out.log_policies.backward(GL)
    g = c.grad
    assert _zero(g[outside[:, 0]])
    ref, ever = PO.soft_policy_grads(wc, wg, wp, None, GL[win].cpu().numpy(), tau, K)
    assert np.abs(ref).max() > 0
    _check_grad(g[(slice(None),) + TC.CORNER_WINDOW], ref, ever, "far corner")


# ---- 6: a BAD_COST map between two good ones ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [float("nan"), -0.25])
def test_one_bad_cost_map_between_two_good_ones(value):
    from neural_astar import ops
    (H, W, _, _), _ = _seam_shapes()
    K, tau = 40, 0.3
    cost, passable, goal = (a.copy() for a in TC.maps(H, W, 3, 41))
    cost[1][tuple(np.argwhere(passable[1] != 0)[-7])] = value       # in the last tile
    cost[2][tuple(np.argwhere(passable[2] == 0)[0])] = np.nan       # an obstacle's cost is not looked at
    tc, tg, tp = _t(cost), _t(goal), _t(passable)
    out, tape = ops.soft_policy_tiled_forward(tc, tg, tp, tau, K, tape=True)
    assert out.status.tolist() == [0, 9, 0]
    assert bool(torch.isneginf(out.log_policies[1]).all()) and not bool(out.policies[1].any())
    act = torch.isfinite(out.log_policies).cpu().numpy()
    assert act[0].sum() > 100 and act[2].sum() > 100
    rng = np.random.default_rng(3)
    GL, G = _t(np.where(act, rng.standard_normal(act.shape), np.nan)), _t(rng.standard_normal(cost.shape))
    grad, st = ops.soft_policy_tiled_backward(tc, tg, tp, tape, G, GL, tau, K)
    assert st.tolist() == [0, 9, 0] and _zero(grad[1]) and bool(grad[0].any()) and bool(grad[2].any())
    # the neighbours' bits are those they have alone, and those of the one-workgroup kernels
    good = [0, 2]
    alone, tape2 = ops.soft_policy_tiled_forward(tc[good], tg[good], tp[good], tau, K, tape=True)
    grad2, _ = ops.soft_policy_tiled_backward(tc[good], tg[good], tp[good], tape2, G[good], GL[good], tau, K)
    assert _bits(alone.log_policies, out.log_policies[good]) and _bits(alone.dists, out.dists[good]) and _bits(grad2, grad[good])
    ref, ref_tape = ops.soft_policy_forward(tc, tg, tp, tau, K, tape=True)
    assert _bits(out.log_policies, ref.log_policies) and _bits(out.status, ref.status)
    assert _bits(grad, ops.soft_policy_backward(tc, tg, tp, ref_tape, G, GL, tau, K)[0])
    for x in (tc.clone().requires_grad_(True), tc):
        with pytest.raises(ValueError, match=r"map\(s\) \[1\]"):
            ops.soft_policy_tiled(x, tg, tp, tau, K)


# ---- 7: the imitation loss ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", TC.MAXENT_TAUS)
def test_soft_policy_nll_tiled_and_its_gradient(tau):
    from neural_astar import ops
    B, H, W, K = PC.LOSS_B, PC.LOSS_H, PC.LOSS_W, PC.LOSS_K
    cost, passable, goal = PC.loss_maps()
    tg, tp = _t(goal), _t(passable)
    opt = ops.cost_to_go_tiled(_t(cost), tg, tp)[0].policies        # the optimal action of every cell, the dataset's order
    assert tuple(opt.shape) == (B, 8, H, W)
    c = _t(cost)[:, None].requires_grad_(True)
    # map 1 demonstrates 27 moves onto cells with no goal within K - 1 moves: the raw demonstration is refused, naming it
    with pytest.raises(ValueError, match=r"map\(s\) \[1\]"):
        ops.soft_policy_nll_tiled(c, tg[:, None], tp[:, None], opt, tau, K)
    logp, act = PO.log_policies(cost, goal, passable, tau, K)
    lost = PC.shown_outside_act(opt.cpu().numpy(), act)
    assert lost.sum((1, 2)).tolist() == [0, 27]
    w = np.where(lost[:, None], 0, opt.cpu().numpy())
    counted = (act.any(1) & (w != 0).any(1)).sum((1, 2))
    print(f"tau {tau}: counted cells {counted.tolist()}")
    assert (counted > 12000).all()
    nll = ops.soft_policy_nll_tiled(c, tg[:, None], tp[:, None], _t(w), tau, K)
    assert tuple(nll.shape) == (B,) and nll.requires_grad
    ref, dlogp = PO.nll(logp, act, w)
    V = SO.soft_fields(cost, goal, passable, tau, K)[0]
    # a mean of log-probabilities, each inside the forward's bound (the bound of tests/test_soft_policy_gpu.py)
    tol = 2 * SO.FWD_RTOL * np.abs(V[np.isfinite(V)]).max() / tau + 16 * EPS * (1 + np.abs(logp[(w != 0) & act]).max())
    got = nll.detach().cpu().numpy().astype(f64)
    print(f"tau {tau}: nll {got}, against the definition {np.abs(got - ref).max():.3e} (tol {tol:.3e})")
    assert (got > 0).all() and np.abs(got - ref).max() <= tol
    nll.sum().backward()
    want, ever = PO.soft_policy_grads(cost, goal, passable, None, dlogp, tau, K)
    assert tuple(c.grad.shape) == (B, 1, H, W) and bool(c.grad.any())
    _check_grad(c.grad[:, 0], want, ever, f"nll tau={tau}")


# ---- 8: training -------------------------------------------------------------------------------------------------------------------------------------------
def test_neural_astar_trains_its_encoder_on_the_tiled_imitation_loss():
    from neural_astar import ops
    from neural_astar.planner import NeuralAstar, VanillaAstar
    from neural_astar.utils import synthetic as syn
    H = W = 96
    assert H * W > ops.SOFT_FIELDS_GRAD_MAX_CELLS
    Pr = syn.random_obstacle_maps(2, H, W, 0.25, seed=93)
    m, s, g = (_t(a) for a in Pr)
    opt = VanillaAstar().to(_dev()).cost_to_go(m, g).policies
    assert tuple(opt.shape) == (2, 8, H, W) and int(opt.sum()) > 5000          # thousands of supervised cells per map
    torch.manual_seed(0)
    na = NeuralAstar(encoder_arch="CNN").to(_dev()).train()
    nll = na.policy_nll(m, s, g, opt, 0.25, tiled=True)
    assert tuple(nll.shape) == (2,) and bool(torch.isfinite(nll).all()) and bool((nll > 0).all())
    nll.sum().backward()
    grads = [q.grad for q in na.encoder.parameters()]
    assert grads and all(x is not None and bool(torch.isfinite(x).all()) for x in grads) and any(bool(x.any()) for x in grads)
    with pytest.raises(NotImplementedError, match="6144"):
        na.policy_nll(m, s, g, opt, 0.25)
    assert na.soft_policy_tiled(m, s, g, 0.25).log_policies.requires_grad
    with torch.no_grad():
        out = na.soft_policy_tiled(m, s, g, 0.25)
    assert out.log_policies.grad_fn is None and not out.dists.requires_grad and not out.policies.requires_grad
    vout = VanillaAstar().to(_dev()).soft_policy_tiled(m, g, 0.25)
    assert vout.log_policies.grad_fn is None and bool(torch.isfinite(VanillaAstar().to(_dev()).policy_nll(m, g, opt, 0.25, tiled=True)).all())
