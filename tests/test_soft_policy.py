"""CPU: the log-policy of the entropy-regularised cost-to-go field and the gradient through it (include/nastar_soft_policy.h,
``ops.soft_policy``, ``ops.soft_policy_nll``) -- everything that needs no GPU.

1. the fifteenth header against ``_native.SOFT_POLICY_SIGNATURES``; the tables of the other headers are what they were;
2. the library exports the three symbols; every refusal the two entry points make before any HIP call, and their order;
3. the numpy definition (tests/soft_policy_oracle.py): its VJP against central differences of its own float64 log-policy; K = 1 gives
   exactly zero; the log-policy is the log of the policy where that has not underflowed;
4. the float32 restatement's error against float64 on the cases of the GPU tests: the figure ``PO.PGRAD_RTOL`` is 4 x of;
5. the Python refusals made before a launch, and the planner methods.
"""
import inspect

import numpy as np
import pytest
import torch

import heuristic_oracle as HO
import soft_fields_oracle as SO
import soft_policy_oracle as PO
from test_fields import _defines, _prototypes

f32, f64 = np.float32, np.float64
NAMES = ["nastar_soft_policy_abi", "nastar_soft_policy_backward", "nastar_soft_policy_forward"]


# ---- 1, 2: header, binding, library, refusals ----------------------------------------------------------------------------------------------------
def test_fifteenth_header_and_soft_policy_signatures_agree():
    from neural_astar import _native
    protos = _prototypes("nastar_soft_policy.h")
    assert sorted(protos) == sorted(_native.SOFT_POLICY_SIGNATURES) == NAMES
    for name, (ret, args) in protos.items():
        assert _native.SOFT_POLICY_SIGNATURES[name] == ret + " " + "".join(k for k, _ in args), name
    assert [n for _, n in protos["nastar_soft_policy_forward"][1]] == ["cost", "goal", "passable", "B", "H", "W", "neighbor_mask", "tau", "horizon",
                                                                       "dist_out", "policy_out", "log_policy_out", "status_out", "tape",
                                                                       "tape_bytes", "stream"]
    assert [n for _, n in protos["nastar_soft_policy_backward"][1]] == ["cost", "goal", "passable", "tape", "tape_bytes", "grad_dist",
                                                                        "grad_log_policy", "B", "H", "W", "neighbor_mask", "tau", "horizon",
                                                                        "grad_cost_out", "status_out", "stream"]
    # a table of its own: the tables tests/test_capi_library.py counts, and the thirteenth's, are what they were
    for table in (_native.SIGNATURES, _native.FIELD_SIGNATURES, _native.TILED_FIELD_SIGNATURES, _native.SOFT_FIELD_SIGNATURES,
                  _native.SOFT_FIELD_TILED_SIGNATURES):
        assert not set(_native.SOFT_POLICY_SIGNATURES) & set(table)
    assert len(_native.SIGNATURES) == 74 and len(_native.FIELD_SIGNATURES) == 4 and len(_native.TILED_FIELD_SIGNATURES) == 6
    assert len(_native.SOFT_FIELD_SIGNATURES) == 6 and len(_prototypes("nastar_soft_fields.h")) == 6
    assert _defines("nastar_soft_policy.h") == {"NASTAR_SOFT_POLICY_ABI": 1} and _defines("nastar.h")["NASTAR_VERSION"] == 800


def test_library_exports_the_soft_policy_symbols():
    from neural_astar import _native, ops
    lib = _native.load()
    for sym in _native.SOFT_POLICY_SIGNATURES:
        assert hasattr(lib, sym), sym
    assert lib.nastar_soft_policy_abi() == 1
    assert len(lib.nastar_soft_policy_forward.argtypes) == 16 == len(lib.nastar_soft_policy_backward.argtypes)
    assert {"soft_policy", "SoftPolicyOutput", "soft_policy_nll", "soft_policy_forward", "soft_policy_backward"} <= set(ops.__all__)
    assert ops.SoftPolicyOutput._fields == ("dists", "log_policies", "policies", "status")


P = 0x10000  # never dereferenced: every call below is refused on its arguments


def _fwd(**over):
    a = dict(cost=P, goal=P, passable=P, B=2, H=8, W=8, neighbor_mask=0x1EF, tau=0.5, horizon=16, dist_out=P, policy_out=None, log_policy_out=P,
             status_out=P, tape=None, tape_bytes=0, stream=None)
    a.update(over)
    return a


def _bwd(**over):
    a = dict(cost=P, goal=P, passable=P, tape=P, tape_bytes=2 * 64 * 16 * 4, grad_dist=P, grad_log_policy=P, B=2, H=8, W=8, neighbor_mask=0x1EF,
             tau=0.5, horizon=16, grad_cost_out=P, status_out=P, stream=None)
    a.update(over)
    return a


# (the table of tests/test_soft_fields.py: the refusals are those of the thirteenth header's entry points, in the same order)
SHARED = [(dict(neighbor_mask=0x1FF), 2), (dict(neighbor_mask=0x200), 2), (dict(cost=None), 5), (dict(goal=None), 5), (dict(passable=None), 5),
          (dict(status_out=None), 5), (dict(B=0), 1), (dict(H=0), 1), (dict(W=-1), 1), (dict(horizon=0), 1), (dict(horizon=-3), 1),
          (dict(tau=0.0), 1), (dict(tau=-1.0), 1), (dict(tau=float("nan")), 1), (dict(tau=float("inf")), 1),
          (dict(neighbor_mask=0x010, cost=None), 2),      # the mask is looked at first
          (dict(cost=None, B=0), 5),                       # a NULL before the shape
          (dict(tau=0.0, H=128, W=129), 1),                # the shape and tau before the limit
          (dict(H=65536, W=65536), 2)]


@pytest.mark.parametrize("over,rc", SHARED + [
    (dict(dist_out=None), 5), (dict(log_policy_out=None), 5), (dict(log_policy_out=None, B=0), 5),
    (dict(H=96, W=128, tape=P + 4, tape_bytes=0), 6), (dict(H=1, W=12289), 2), (dict(H=97, W=128), 2),
    (dict(H=97, W=128, tape=P, tape_bytes=0), 2),          # the limit before the tape
    (dict(tape=P, tape_bytes=2 * 64 * 16 * 4 - 1), 6), (dict(tape=P + 4, tape_bytes=1 << 20), 6), (dict(tape=P, tape_bytes=0), 6)])
def test_soft_policy_forward_refuses_bad_arguments_without_a_device(over, rc):
    from neural_astar import _native
    lib = _native.load()
    assert lib.nastar_soft_policy_forward(*_fwd(**over).values()) == rc
    assert lib.nastar_soft_policy_forward(*_fwd(**dict(dict(policy_out=P), **over)).values()) == rc
    assert lib.nastar_last_error() == b""


@pytest.mark.parametrize("over,rc", SHARED + [
    (dict(tape=None), 5), (dict(grad_cost_out=None), 5), (dict(H=64, W=97), 2), (dict(H=1, W=6145), 2),
    (dict(H=64, W=97, tape_bytes=0), 2),                   # the limit before the tape
    (dict(tape_bytes=2 * 64 * 16 * 4 - 1), 6), (dict(tape=P + 8), 6), (dict(horizon=17), 6), (dict(B=3), 6)])
def test_soft_policy_backward_refuses_bad_arguments_without_a_device(over, rc):
    from neural_astar import _native
    lib = _native.load()
    for seeds in (dict(), dict(grad_dist=None), dict(grad_log_policy=None), dict(grad_dist=None, grad_log_policy=None)):   # either may be NULL
        assert lib.nastar_soft_policy_backward(*_bwd(**dict(seeds, **over)).values()) == rc
    assert lib.nastar_last_error() == b""


# ---- 3: the definition -------------------------------------------------------------------------------------------------------------------------------
FD_CASES = [(5, 7, HO.MOORE8, 11), (6, 6, HO.VON_NEUMANN, 12), (4, 9, HO.MOORE8, 13)]


@pytest.mark.parametrize("H,W,mask,seed", FD_CASES)
@pytest.mark.parametrize("tau", [1.0, 0.3])
def test_oracle_vjp_is_the_central_difference_of_its_own_log_policy(H, W, mask, seed, tau):
    K, h = 30, 2.0 ** -10                                          # (the oracle casts costs to float32: the step is exact there)
    cost, passable, goal = (a[0] for a in SO.random_maps(seed, 1, H, W))
    cost = np.round(cost * 2 ** 10) / 2 ** 10 + f32(2.0 ** -9)      # costs on the grid of the step, all above it
    lp = PO.log_policy(cost, goal, passable, tau, K, mask)
    assert lp.act.sum() > 8 and np.array_equal(np.isfinite(lp.logp), lp.act)
    rng = np.random.default_rng(seed)
    GL, G = PO.upstream(seed, lp.act), rng.standard_normal((H, W))
    got = PO.soft_policy_grad(cost, goal, passable, None, GL, tau, K, mask)
    both = PO.soft_policy_grad(cost, goal, passable, G, GL, tau, K, mask)
    assert np.array_equal(both.grad, both.field_part + got.grad) and got.policy_part.any() and not got.field_part.any()
    weight = np.where(lp.act, GL, 0.0)
    fd = np.zeros((H, W))
    for y, x in np.argwhere(passable != 0):
        up, dn = cost.copy(), cost.copy()
        up[y, x] += f32(h)
        dn[y, x] -= f32(h)
        a, b = PO.log_policy(up, goal, passable, tau, K, mask), PO.log_policy(dn, goal, passable, tau, K, mask)
        assert np.array_equal(a.act, lp.act) and np.array_equal(b.act, lp.act)
        fd[y, x] = (weight * (np.where(lp.act, a.logp, 0.0) - np.where(lp.act, b.logp, 0.0))).sum() / (2 * h)
    err = np.abs(got.grad - fd).max() / np.abs(fd).max()
    print(f"{H}x{W} mask {mask:#05x} tau {tau}: VJP against central differences, rel {err:.3e}")
    assert err <= 1e-4                                              # the differences' own h^2 term; a wrong formula is off by O(1)
    assert not got.grad[~got.ever].any()


@pytest.mark.parametrize("mask", SO.MASKS)
def test_horizon_one_has_no_gradient_through_the_policy(mask):
    cost, passable, goal = (a[0] for a in SO.random_maps(21, 1, 7, 8))
    for y, x in ((0, 0), (3, 4)):
        passable[y, x] = goal[y, x] = 1                             # several goals: several cells are live at K = 1
    lp = PO.log_policy(cost, goal, passable, 0.3, 1, mask)
    assert lp.act.any()
    for dtype in (f64, f32):
        g = PO.soft_policy_grad(cost, goal, passable, None, PO.upstream(3, lp.act), 0.3, 1, mask, dtype)
        assert not g.grad.any() and not g.policy_part.any()


@pytest.mark.parametrize("tau", SO.TAUS)
def test_log_policy_is_the_log_of_the_policy_and_finite_where_that_underflows(tau):
    cost, passable, goal = (a[0] for a in SO.random_maps(31, 1, 12, 13, hi=4.0))   # (cost / tau up to 200 per step at the small tau)
    K = SO.default_horizon(12, 13)
    lp = PO.log_policy(cost, goal, passable, tau, K)
    pol = lp.field.policy
    live = (passable != 0) & (goal == 0) & np.isfinite(lp.field.dist)
    assert np.array_equal(lp.act.any(0), live) and not lp.act[:, ~live].any()
    assert np.abs(np.exp(lp.logp) - pol).max() <= 1e-14 and np.abs(np.exp(lp.logp).sum(0)[live] - 1).max() <= 1e-13
    if tau == 0.02:                                                 # float32 probabilities underflow here; the log-policy does not
        small = lp.act & (lp.logp < np.log(2.0 ** -149))
        assert small.any() and np.isfinite(PO.log_policy(cost, goal, passable, tau, K, dtype=f32).logp[small]).all()
    bad = cost.copy()
    bad[tuple(np.argwhere(passable != 0)[2])] = np.nan
    none = PO.log_policy(bad, goal, passable, tau, K)
    assert none.field.status == SO.STATUS_BAD_COST and np.isneginf(none.logp).all() and not none.act.any()
    assert not PO.soft_policy_grad(bad, goal, passable, np.ones((12, 13)), np.ones((8, 12, 13)), tau, K).grad.any()


# ---- 4: the float32 restatement: the scale of the gradient's bound ----------------------------------------------------------------------------------
def test_float32_restatement_of_the_policy_gradient():
    """the float32 restatement of the VJP against float64 on the cases of the GPU tests, with the seed GL alone and with both seeds: the
    figure tests/soft_policy_oracle.py commits 4 x of as PGRAD_RTOL"""
    worst = 0.0
    for H, W, B, seed in SO.SHAPE_CASES:
        cost, passable, goal = SO.random_maps(seed, B, H, W)
        for K, tau, mask in SO.sweep_cases(goal[0], passable[0]):
            act = PO.log_policy(cost[0], goal[0], passable[0], tau, K, mask).act
            assert np.array_equal(act, PO.log_policy(cost[0], goal[0], passable[0], tau, K, mask, f32).act)
            GL = PO.upstream(seed, act)
            G = np.random.default_rng(seed + 100).standard_normal((H, W))
            a = PO.soft_policy_grad(cost[0], goal[0], passable[0], G, GL, tau, K, mask)
            b = PO.soft_policy_grad(cost[0], goal[0], passable[0], G, GL, tau, K, mask, f32)
            worst = max(worst, SO.rel_err(b.policy_part, a.policy_part), SO.rel_err(b.grad, a.grad))   # GL alone; GL and G
    print(f"float32 restatement of the policy gradient: {worst:.3e}; PGRAD_RTOL = {PO.PGRAD_RTOL:.3e}")
    assert 0 < worst <= PO.PGRAD_RTOL


# ---- 5: Python refusals before a launch; the planner methods ----------------------------------------------------------------------------------------
def test_refusals_before_a_launch_and_the_planner_methods():
    from neural_astar import ops
    from neural_astar.planner import NeuralAstar, VanillaAstar
    from neural_astar.planner.differentiable_astar import DifferentiableAstar
    assert list(inspect.signature(ops.soft_policy).parameters) == ["cost_maps", "goal_maps", "obstacles_maps", "tau", "horizon", "neighbor_mask"]
    assert list(inspect.signature(ops.soft_policy_nll).parameters) == ["cost_maps", "goal_maps", "obstacles_maps", "opt_policies", "tau", "horizon",
                                                                       "neighbor_mask"]
    for cls in (DifferentiableAstar, VanillaAstar, NeuralAstar):
        assert inspect.signature(cls.soft_policy).parameters["horizon"].default is None, cls
        assert "opt_policies" in inspect.signature(cls.policy_nll).parameters, cls
    m = torch.ones(2, 1, 8, 8, requires_grad=True)
    opt = torch.zeros(2, 8, 8, 8)
    # opt_policies is looked at before anything else could be launched: a wrong shape, a wrong device
    for wrong in (torch.zeros(2, 8, 8, 9), torch.zeros(2, 9, 8, 8), torch.zeros(3, 8, 8, 8), torch.zeros(2, 8, 64), None):
        with pytest.raises(ValueError, match="opt_policies"):
            ops.soft_policy_nll(m, m, m, wrong, 0.5)
    with pytest.raises(ValueError, match="opt_policies"):
        ops.soft_policy_nll(m, m, m, torch.zeros(2, 8, 8, 8, device="meta"), 0.5)
    for tau in (0.0, -0.5, float("nan"), float("inf"), True, None):
        with pytest.raises(ValueError, match="tau"):
            ops.soft_policy(m, m, m, tau)
        with pytest.raises(ValueError, match="tau"):
            ops.soft_policy_nll(m, m, m, opt, tau)
    with pytest.raises(ValueError, match="horizon"):
        ops.soft_policy(m, m, m, 0.5, horizon=0)
    with pytest.raises(ValueError, match="neighbor_mask"):
        ops.soft_policy(m, m, m, 0.5, neighbor_mask=0x1FF)
    with pytest.raises(ValueError, match="share one"):
        ops.soft_policy(m, torch.ones(2, 1, 8, 9), m, 0.5)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.soft_policy(m, m, m, 0.5)
    big = torch.ones(1, 1, 64, 97, requires_grad=True)            # above the backward's limit, below the forward's
    with pytest.raises(NotImplementedError, match="6144"):
        ops.soft_policy(big, big, big, 0.5)
    with pytest.raises(RuntimeError, match="HIP device"):         # ... the evaluation call takes it
        ops.soft_policy(big.detach(), big.detach(), big.detach(), 0.5)
    huge = torch.ones(1, 1, 97, 128)
    with pytest.raises(NotImplementedError, match="12288"):
        ops.soft_policy(huge, huge, huge, 0.5)
    with pytest.raises(NotImplementedError, match="6144"):
        ops.soft_policy_backward(big, big, big, torch.zeros(8, dtype=torch.uint8), None, None, 0.5)
    with pytest.raises(ValueError, match="grad_log_policies"):
        ops.soft_policy_backward(m, m, m, torch.zeros(8, dtype=torch.uint8), None, torch.zeros(2, 8, 8, 9), 0.5)
    with pytest.raises(ValueError, match="tau"):
        VanillaAstar().soft_policy(m, m, 0.0)
    with pytest.raises(ValueError, match="tau"):
        NeuralAstar().policy_nll(m, m, m, opt, -1.0)
    with pytest.raises(RuntimeError, match="HIP device"):
        DifferentiableAstar().policy_nll(m, m, m, opt, 0.5)
