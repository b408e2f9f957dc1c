"""GPU: the log-policy of the entropy-regularised cost-to-go field and the gradient through it (include/nastar_soft_policy.h,
``ops.soft_policy``, ``ops.soft_policy_nll``) against the float64 definition of tests/soft_policy_oracle.py -- never against the kernels' own
output, except where the header promises the BITS of the thirteenth header's kernels.  The maps are those of tests/test_soft_fields_gpu.py:
25 % obstacles, costs U(0.1, 1).  Where -inf lies must match exactly; a finite log-probability is held to
``2 * SO.FWD_RTOL * max|V| / tau + 16 * 2**-24 * (1 + |logpi|)`` (a difference of two plane values over tau: the bound of the existing policy
check) and a gradient to ``PO.PGRAD_RTOL`` of the case's max |gradient|; the figures are printed before they are asserted.
"""
import functools

import numpy as np
import pytest
import torch

import soft_fields_oracle as SO
import soft_policy_oracle as PO

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
MOORE8 = SO.MOORE8
EPS = 2.0 ** -24


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, f32)).to(_dev())


def _bits(t):
    return t.contiguous().view(torch.uint8)


@functools.lru_cache(maxsize=None)
def _maps(H, W, B, seed):
    return SO.random_maps(seed, B, H, W)


def _check_log_policy(out, cost, passable, goal, tau, K, mask, what):
    """the log-policy against the definition -> (the definition's logp, act)"""
    ref, act = PO.log_policies(cost, goal, passable, tau, K, mask)
    lp = out.log_policies.detach().cpu().numpy()
    assert not np.isnan(lp).any() and np.array_equal(np.isfinite(lp), act) and (lp[~act] == -np.inf).all(), what   # where -inf lies: exactly
    if act.any():
        V = SO.soft_fields(cost, goal, passable, tau, K, mask)[0]
        scale = np.abs(V[np.isfinite(V)]).max()
        tol = 2 * SO.FWD_RTOL * scale / tau + 16 * EPS * (1 + np.abs(ref[act]))
        err = np.abs(lp[act].astype(f64) - ref[act])
        print(f"{what}: log-policy err {err.max():.3e} (tol at that entry {tol[err.argmax()]:.3e}), smallest logpi {ref[act].min():.1f}")
        assert (err <= tol).all(), what
        p = out.policies.cpu().numpy().astype(f64)
        with np.errstate(under="ignore"):
            back = np.abs(np.exp(lp.astype(f64)) - p).max()
        print(f"{what}: exp(log-policy) against the policy {back:.3e}")
        assert back <= 16 * EPS, what
    return ref, act


def _check_grad(grad, ref, ever, what):
    g = grad.cpu().numpy()
    assert np.isfinite(g).all(), what
    never = g[~ever]
    assert not never.any() and not np.signbit(never).any(), what                                 # +0.0f, bit for bit
    err = SO.rel_err(g, ref)
    print(f"{what}: gradient rel err {err:.3e} (bound {PO.PGRAD_RTOL:.3e})")
    assert err <= PO.PGRAD_RTOL, what


# ---- the shapes, horizons, temperatures and move sets where the kernels can go wrong ----------------------------------------------------------
@pytest.mark.parametrize("H,W,B,seed", SO.SHAPE_CASES, ids=lambda v: str(v))
def test_log_policy_and_its_gradient_are_the_definition(H, W, B, seed):
    from neural_astar import ops
    cost, passable, goal = _maps(H, W, B, seed)
    c, g, p = _t(cost), _t(goal), _t(passable)
    for K, tau, mask in SO.sweep_cases(goal[0], passable[0]):
        what = f"{B}x{H}x{W} K={K} tau={tau} mask={mask:#05x}"
        out, tape = ops.soft_policy_forward(c, g, p, tau, K, mask, policies=True, tape=True)
        old, old_tape = ops.soft_fields_forward(c, g, p, tau, K, mask, policies=True, tape=True)
        for a, b in ((out.dists, old.dists), (out.policies, old.policies), (out.status, old.status), (tape, old_tape)):
            assert torch.equal(_bits(a), _bits(b)), what                                         # the thirteenth header's bits
        nopol, _ = ops.soft_policy_forward(c, g, p, tau, K, mask, policies=False)
        assert nopol.policies is None and torch.equal(_bits(nopol.log_policies), _bits(out.log_policies)), what
        _, act = _check_log_policy(out, cost, passable, goal, tau, K, mask, what)
        # the gradient: a NaN on every entry of GL outside (live at K, Act), and on every cell of G that is not live at K
        GL = PO.upstream(seed, act)
        G = np.where(act.any(1), np.random.default_rng(seed + 100).standard_normal((B, H, W)), np.nan)
        parts = [PO.soft_policy_grad(cost[b], goal[b], passable[b], G[b], GL[b], tau, K, mask) for b in range(B)]
        ever = np.stack([q.ever for q in parts])
        alone, _ = ops.soft_policy_backward(c, g, p, tape, None, _t(GL), tau, K, mask)
        _check_grad(alone, np.stack([q.policy_part for q in parts]), ever, what + " GL alone")
        both, st = ops.soft_policy_backward(c, g, p, old_tape, _t(G), _t(GL), tau, K, mask)      # (either forward's tape)
        _check_grad(both, np.stack([q.grad for q in parts]), ever, what + " GL and G")
        assert st.tolist() == [0] * B
        field, _ = ops.soft_policy_backward(c, g, p, tape, _t(G), None, tau, K, mask)
        assert torch.equal(_bits(field), _bits(ops.soft_fields_backward(c, g, p, tape, _t(G), tau, K, mask)[0])), what
        none, _ = ops.soft_policy_backward(c, g, p, tape, None, None, tau, K, mask)
        assert not none.any() and not torch.signbit(none).any(), what
        if K == 1:
            assert not alone.any() and not torch.signbit(alone).any() and torch.equal(_bits(both), _bits(field)), what   # exactly 0.0f


def test_two_calls_agree_bit_for_bit_forward_and_backward():
    from neural_astar import ops
    H, W, B, K, tau = 40, 50, 24, 96, 0.1                           # 2000 cells: four wavefronts per map, several maps per CU
    cost, passable, goal = _maps(H, W, B, 61)
    rng = np.random.default_rng(0)
    G, GL = _t(rng.standard_normal(cost.shape)), _t(rng.standard_normal((B, 8, H, W)))
    runs = []
    for _ in range(2):
        out, tape = ops.soft_policy_forward(_t(cost), _t(goal), _t(passable), tau, K, policies=True, tape=True)
        grad, _ = ops.soft_policy_backward(_t(cost), _t(goal), _t(passable), tape, G, GL, tau, K)
        runs.append((out.dists, out.log_policies, out.policies, tape, grad))
    for a, b in zip(*runs):
        assert torch.equal(_bits(a), _bits(b))
    assert bool(runs[0][4].any())


# ---- the limits ---------------------------------------------------------------------------------------------------------------------------------
def test_backward_limit_exactly_and_one_cell_more_is_refused():
    from neural_astar import _native, ops
    H, W = 64, 96                                                  # the full LDS, six cells per lane
    assert H * W == ops.SOFT_FIELDS_GRAD_MAX_CELLS == _native.load().nastar_soft_fields_grad_max_cells()
    cost, passable, goal = _maps(H, W, 2, 32)
    K, tau = 2 * (H + W), 0.1
    c = _t(cost).requires_grad_(True)
    out = ops.soft_policy(c, _t(goal), _t(passable), tau, K)
    assert out.dists.requires_grad and out.log_policies.requires_grad and not out.policies.requires_grad
    _, act = _check_log_policy(out, cost, passable, goal, tau, K, MOORE8, "backward limit")
    GL = PO.upstream(32, act)
    G = np.where(act.any(1), np.random.default_rng(33).standard_normal(cost.shape), np.nan)
    torch.autograd.backward([out.dists, out.log_policies], [_t(G)[:, None], _t(GL)])            # ONE node, one launch
    ref, ever = PO.soft_policy_grads(cost, goal, passable, G, GL, tau, K)
    _check_grad(c.grad, ref, ever, "backward limit")
    wide = torch.ones(1, 64, 97, device=_dev(), requires_grad=True)
    with pytest.raises(NotImplementedError, match="6144"):
        ops.soft_policy(wide, wide, wide, 0.5)
    st = torch.empty(1, dtype=torch.int32, device=_dev())
    ptr = wide.data_ptr()
    rc = _native.load().nastar_soft_policy_backward(ptr, ptr, ptr, ptr, 1 << 40, None, None, 1, 1, 6145, MOORE8, 0.5, 4, ptr, st.data_ptr(),
                                                    torch.cuda.current_stream(_dev()).cuda_stream)
    assert rc == _native.NASTAR_ERR_UNSUPPORTED


def test_one_node_two_outputs_and_no_graph_without_a_gradient():
    from neural_astar import ops
    H, W = 9, 11
    cost, passable, goal = _maps(H, W, 2, 21)
    c = _t(cost)[:, None].requires_grad_(True)
    g, p = _t(goal)[:, None], _t(passable)[:, None]
    out = ops.soft_policy(c, g, p, 0.5)                             # the default horizon
    assert out.dists.grad_fn is not None and out.dists.grad_fn is out.log_policies.grad_fn
    assert tuple(out.dists.shape) == (2, 1, H, W) and tuple(out.log_policies.shape) == (2, 8, H, W) == tuple(out.policies.shape)
    _check_log_policy(out, cost, passable, goal, 0.5, 2 * (H + W), MOORE8, "default horizon")
    with torch.no_grad():
        quiet = ops.soft_policy(c, g, p, 0.5)
    assert quiet.log_policies.grad_fn is None and not quiet.dists.requires_grad
    assert ops.soft_policy(c.detach(), g, p, 0.5).log_policies.grad_fn is None
    assert torch.equal(_bits(quiet.log_policies), _bits(out.log_policies))
    # the log-policy alone: [B,1,H,W] in, [B,1,H,W] gradient out; the -inf VALUES are masked by the loss
    lp = out.log_policies
    torch.where(torch.isfinite(lp), lp, torch.zeros_like(lp)).sum().backward()
    assert tuple(c.grad.shape) == (2, 1, H, W) and bool(c.grad.any()) and bool(torch.isfinite(c.grad).all())


# ---- a BAD_COST map between two good ones ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [float("nan"), -0.25])
def test_one_bad_cost_map_between_two_good_ones(value):
    from neural_astar import ops
    H, W, K, tau = 7, 9, 20, 0.3
    cost, passable, goal = (a.copy() for a in _maps(H, W, 3, 41))
    cost[1][tuple(np.argwhere(passable[1] != 0)[5])] = value
    cost[2][tuple(np.argwhere(passable[2] == 0)[0])] = np.nan      # an obstacle's cost is not looked at
    c, g, p = _t(cost), _t(goal), _t(passable)
    out, tape = ops.soft_policy_forward(c, g, p, tau, K, policies=True, tape=True)
    assert out.status.tolist() == [0, 9, 0]
    _, act = _check_log_policy(out, cost, passable, goal, tau, K, MOORE8, "bad cost")
    assert bool(torch.isneginf(out.log_policies[1]).all()) and not out.policies[1].any() and act[0].any() and act[2].any() and not act[1].any()
    rng = np.random.default_rng(3)
    GL, G = np.where(act, rng.standard_normal(act.shape), np.nan), rng.standard_normal(cost.shape)
    grad, st = ops.soft_policy_backward(c, g, p, tape, _t(G), _t(GL), tau, K)
    assert st.tolist() == [0, 9, 0] and not grad[1].any()
    ref, ever = PO.soft_policy_grads(cost, goal, passable, G, GL, tau, K)
    _check_grad(grad, ref, ever, "bad cost")
    with pytest.raises(ValueError, match=r"map\(s\) \[1\]"):
        ops.soft_policy(c.requires_grad_(True), g, p, tau, K)
    with pytest.raises(ValueError, match=r"map\(s\) \[1\]"):
        ops.soft_policy(c.detach(), g, p, tau, K)


# ---- the imitation loss ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", SO.TAUS)
def test_soft_policy_nll_and_its_gradient(tau):
    from neural_astar import ops
    B, H, W = 4, 16, 16
    cost, passable, goal = _maps(H, W, B, 81)
    K = 2 * (H + W)
    opt = ops.cost_to_go(_t(cost), _t(goal), _t(passable)).policies   # the optimal action of every cell, the dataset's order
    assert tuple(opt.shape) == (B, 8, H, W) and int(opt.sum()) > B * 40
    c = _t(cost)[:, None].requires_grad_(True)
    nll = ops.soft_policy_nll(c, _t(goal)[:, None], _t(passable)[:, None], opt, tau)
    assert tuple(nll.shape) == (B,) and nll.requires_grad
    logp, act = PO.log_policies(cost, goal, passable, tau, K)
    w = opt.cpu().numpy()
    ref, dlogp = PO.nll(logp, act, w)
    V = SO.soft_fields(cost, goal, passable, tau, K)[0]
    # a mean of log-probabilities, each inside the forward's bound
    tol = 2 * SO.FWD_RTOL * np.abs(V[np.isfinite(V)]).max() / tau + 16 * EPS * (1 + np.abs(logp[(w != 0) & act]).max())
    got = nll.detach().cpu().numpy().astype(f64)
    print(f"tau {tau}: nll {got}, against the definition {np.abs(got - ref).max():.3e} (tol {tol:.3e})")
    assert (got > 0).all() and np.abs(got - ref).max() <= tol
    nll.sum().backward()
    want, ever = PO.soft_policy_grads(cost, goal, passable, None, dlogp, tau, K)
    _check_grad(c.grad[:, 0], want, ever, f"nll tau={tau}")
    assert bool(c.grad.any())
    # a map with no counted cell gives 0; a demonstrated move into an obstacle is named
    none = opt.clone()
    none[1] = 0
    assert ops.soft_policy_nll(c.detach(), _t(goal), _t(passable), none, tau)[1].item() == 0.0
    b = 2
    y, x = next((y, x) for y, x in np.argwhere(act[b].any(0)) if x + 1 < W and passable[b, y, x + 1] == 0)
    wrong = opt.clone()
    wrong[b, :, y, x] = 0
    wrong[b, 1, y, x] = 1                                            # action 1 = (0, 1): onto the obstacle to the right
    with pytest.raises(ValueError, match=r"map\(s\) \[2\]"):
        ops.soft_policy_nll(c, _t(goal), _t(passable), wrong, tau)


def test_neural_astar_trains_its_encoder_on_the_imitation_loss():
    from neural_astar.planner import NeuralAstar, VanillaAstar
    from neural_astar.utils import synthetic as syn
    Pr = syn.random_obstacle_maps(2, 32, 32, 0.25, seed=91)
    m, s, g = (_t(a) for a in Pr)
    opt = VanillaAstar().to(_dev()).cost_to_go(m, g).policies
    assert tuple(opt.shape) == (2, 8, 32, 32) and int(opt.sum()) > 500      # hundreds of supervised cells per map
    torch.manual_seed(0)
    na = NeuralAstar(encoder_arch="CNN").to(_dev()).train()
    nll = na.policy_nll(m, s, g, opt, 0.25)
    assert tuple(nll.shape) == (2,) and bool(torch.isfinite(nll).all()) and bool((nll > 0).all())
    nll.sum().backward()
    grads = [q.grad for q in na.encoder.parameters()]
    assert grads and all(x is not None and bool(torch.isfinite(x).all()) for x in grads) and any(bool(x.any()) for x in grads)
    assert na.soft_policy(m, s, g, 0.25).log_policies.requires_grad
    with torch.no_grad():
        out = na.soft_policy(m, s, g, 0.25)
    assert out.log_policies.grad_fn is None and not out.dists.requires_grad and not out.policies.requires_grad
    vout = VanillaAstar().to(_dev()).soft_policy(m, g, 0.25)
    assert vout.log_policies.grad_fn is None and bool(torch.isfinite(VanillaAstar().to(_dev()).policy_nll(m, g, opt, 0.25)).all())
