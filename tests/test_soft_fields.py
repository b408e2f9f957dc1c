"""CPU: the entropy-regularised cost-to-go field over a finite horizon and its gradient (include/nastar_soft_fields.h,
``ops.soft_cost_to_go``, ``ops.maxent_path_nll``) -- everything that needs no GPU.

1. the thirteenth header against ``_native.SOFT_FIELD_SIGNATURES``; the tables of the other headers are what they were;
2. the library exports the six symbols; abi and limits; ``tape_bytes`` is monotone in B and in the horizon;
3. every refusal the two entry points make before any HIP call, and their order;
4. the numpy definition (tests/soft_fields_oracle.py) against ``torch.logsumexp`` and torch autograd in float64;
5. the sandwich D - K tau ln(moves) <= V_K <= D against the exact field, and V_K = +inf exactly where no goal lies within K hops;
6. the negative log-likelihood of a demonstration is >= 0; the float32 restatement stays inside the committed bounds;
7. the Python refusals made before a launch, and the planner methods;
8. the signatures of the family's public functions and of the planners' soft methods, as literal strings.
"""
import inspect
import math

import numpy as np
import pytest
import torch

import fields_grad_oracle as GO
import fields_oracle as FO
import heuristic_oracle as HO
import path_masks_oracle as PO
import soft_fields_oracle as SO
from test_fields import _defines, _prototypes

f32, f64 = np.float32, np.float64
NAMES = ["nastar_soft_cost_to_go", "nastar_soft_fields_abi", "nastar_soft_fields_backward", "nastar_soft_fields_grad_max_cells",
         "nastar_soft_fields_max_cells", "nastar_soft_fields_tape_bytes"]


# ---- 1, 2: header, binding, library ---------------------------------------------------------------------------------------------------------------
def test_thirteenth_header_and_soft_field_signatures_agree():
    from neural_astar import _native
    protos = _prototypes("nastar_soft_fields.h")
    assert sorted(protos) == sorted(_native.SOFT_FIELD_SIGNATURES) == NAMES
    for name, (ret, args) in protos.items():
        assert _native.SOFT_FIELD_SIGNATURES[name] == ret + " " + "".join(k for k, _ in args), name
    assert [n for _, n in protos["nastar_soft_cost_to_go"][1]] == ["cost", "goal", "passable", "B", "H", "W", "neighbor_mask", "tau", "horizon",
                                                                   "dist_out", "policy_out", "status_out", "tape", "tape_bytes", "stream"]
    assert [n for _, n in protos["nastar_soft_fields_backward"][1]] == ["cost", "goal", "passable", "tape", "tape_bytes", "grad_dist", "B", "H", "W",
                                                                        "neighbor_mask", "tau", "horizon", "grad_cost_out", "status_out", "stream"]
    # a table of its own: none of the new symbols is a nastar_cost_to_go*, and the tables tests/test_capi_library.py counts are what they were
    assert not [n for n in _native.SOFT_FIELD_SIGNATURES if n.startswith("nastar_cost_to_go")]
    for table in (_native.SIGNATURES, _native.FIELD_SIGNATURES, _native.TILED_FIELD_SIGNATURES, _native.FIELD_GRAD_SIGNATURES):
        assert not set(_native.SOFT_FIELD_SIGNATURES) & set(table)
    assert len(_native.SIGNATURES) == 74 and len(_native.FIELD_SIGNATURES) == 4 and len(_native.TILED_FIELD_SIGNATURES) == 6
    assert len(_prototypes("nastar.h")) == 74
    new = _defines("nastar_soft_fields.h")
    assert new == {"NASTAR_SOFT_FIELDS_ABI": 1} and _defines("nastar.h")["NASTAR_VERSION"] == 800   # no new code, no new version
    assert (SO.STATUS_NO_GOAL, SO.STATUS_BAD_COST) == (_native.NASTAR_ERR_UNSOLVABLE, _native.NASTAR_ERR_BAD_COST) == (3, 9)


def test_library_exports_the_soft_field_symbols():
    from neural_astar import _native, ops
    lib = _native.load()
    for sym in _native.SOFT_FIELD_SIGNATURES:
        assert hasattr(lib, sym), sym
    assert lib.nastar_soft_fields_abi() == 1
    assert lib.nastar_soft_fields_max_cells() == ops.SOFT_FIELDS_MAX_CELLS >= 8192
    assert lib.nastar_soft_fields_grad_max_cells() == ops.SOFT_FIELDS_GRAD_MAX_CELLS >= 4096
    assert ops.SOFT_FIELDS_GRAD_MAX_CELLS <= ops.SOFT_FIELDS_MAX_CELLS
    assert len(lib.nastar_soft_cost_to_go.argtypes) == 15 == len(lib.nastar_soft_fields_backward.argtypes)
    assert {"soft_cost_to_go", "SoftFieldOutput", "maxent_path_nll", "soft_fields_backward"} <= set(ops.__all__)


def test_tape_bytes_is_the_product_and_monotone():
    from neural_astar import _native
    size = _native.load().nastar_soft_fields_tape_bytes
    assert size(3, 5, 7, 24) == 3 * 5 * 7 * 24 * 4
    for B, H, W, K in [(1, 1, 1, 1), (2, 32, 33, 130), (4096, 64, 64, 64)]:
        assert size(B, H, W, K) < size(B + 1, H, W, K) and size(B, H, W, K) < size(B, H, W, K + 1)
    assert [size(0, 4, 4, 4), size(4, 0, 4, 4), size(4, 4, -1, 4), size(4, 4, 4, 0)] == [0, 0, 0, 0]
    big = 2 ** 31 - 1
    assert size(big, 96, 128, big) == 2 ** 64 - 1      # does not fit: no tape is that large


# ---- 3: refusals, made before any HIP call -----------------------------------------------------------------------------------------------------------
P = 0x10000  # never dereferenced: every call below is refused on its arguments


def _fwd(**over):
    a = dict(cost=P, goal=P, passable=P, B=2, H=8, W=8, neighbor_mask=0x1EF, tau=0.5, horizon=16, dist_out=P, policy_out=None, status_out=P,
             tape=None, tape_bytes=0, stream=None)
    a.update(over)
    return a


def _bwd(**over):
    a = dict(cost=P, goal=P, passable=P, tape=P, tape_bytes=2 * 64 * 16 * 4, grad_dist=P, B=2, H=8, W=8, neighbor_mask=0x1EF, tau=0.5, horizon=16,
             grad_cost_out=P, status_out=P, stream=None)
    a.update(over)
    return a


SHARED = [(dict(neighbor_mask=0x1FF), 2), (dict(neighbor_mask=0x200), 2), (dict(cost=None), 5), (dict(goal=None), 5), (dict(passable=None), 5),
          (dict(status_out=None), 5), (dict(B=0), 1), (dict(H=0), 1), (dict(W=-1), 1), (dict(horizon=0), 1), (dict(horizon=-3), 1),
          (dict(tau=0.0), 1), (dict(tau=-1.0), 1), (dict(tau=float("nan")), 1), (dict(tau=float("inf")), 1),
          (dict(neighbor_mask=0x010, cost=None), 2),      # the mask is looked at first
          (dict(cost=None, B=0), 5),                       # a NULL before the shape
          (dict(tau=0.0, H=128, W=129), 1),                # the shape and tau before the limit
          (dict(H=65536, W=65536), 2)]


@pytest.mark.parametrize("over,rc", SHARED + [
    (dict(dist_out=None), 5), (dict(H=96, W=128, tape=P + 4, tape_bytes=0), 6), (dict(H=1, W=12289), 2), (dict(H=97, W=128), 2),
    (dict(H=97, W=128, tape=P, tape_bytes=0), 2),          # the limit before the tape
    (dict(tape=P, tape_bytes=2 * 64 * 16 * 4 - 1), 6), (dict(tape=P + 4, tape_bytes=1 << 20), 6), (dict(tape=P, tape_bytes=0), 6)])
def test_soft_cost_to_go_refuses_bad_arguments_without_a_device(over, rc):
    from neural_astar import _native
    lib = _native.load()
    assert lib.nastar_soft_cost_to_go(*_fwd(**over).values()) == rc
    assert lib.nastar_soft_cost_to_go(*_fwd(**dict(dict(policy_out=P), **over)).values()) == rc
    assert lib.nastar_last_error() == b""


@pytest.mark.parametrize("over,rc", SHARED + [
    (dict(tape=None), 5), (dict(grad_dist=None), 5), (dict(grad_cost_out=None), 5), (dict(H=64, W=97), 2), (dict(H=1, W=6145), 2),
    (dict(H=64, W=97, tape_bytes=0), 2),                   # the limit before the tape
    (dict(tape_bytes=2 * 64 * 16 * 4 - 1), 6), (dict(tape=P + 8), 6), (dict(horizon=17), 6), (dict(B=3), 6)])
def test_soft_fields_backward_refuses_bad_arguments_without_a_device(over, rc):
    from neural_astar import _native
    lib = _native.load()
    assert lib.nastar_soft_fields_backward(*_bwd(**over).values()) == rc
    assert lib.nastar_last_error() == b""


# ---- 4: the definition against torch in float64 ----------------------------------------------------------------------------------------------------
def _torch_field(cost, goal, passable, tau, K, mask):
    """the recursion once more, on ``torch.logsumexp``: cost [H,W] float64 tensor -> V_K [H,W] (goals on obstacles 0, as the output)"""
    H, W = cost.shape
    ok, gl = torch.from_numpy(np.asarray(passable) != 0), torch.from_numpy(np.asarray(goal) != 0)
    inf = torch.full((H, W), math.inf, dtype=torch.float64)
    V = torch.where(gl & ok, torch.zeros_like(inf), inf)
    for _ in range(K):
        pad = torch.nn.functional.pad(V, (1, 1, 1, 1), value=math.inf)
        X = torch.stack([pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy, dx in HO.offsets(mask)])
        fin = torch.isfinite(X).any(0)
        X = torch.where(fin, X, torch.zeros_like(X))            # (a column of +inf alone would be a NaN in logsumexp's backward)
        soft = torch.where(fin, -tau * torch.logsumexp(-X / tau, 0), inf)
        V = torch.where(gl & ok, torch.zeros_like(inf), torch.where(ok, cost + soft, inf))
    return torch.where(gl, torch.zeros_like(inf), V)


def _issue_map():
    """9x11, two goals, one of them on an obstacle, zero costs allowed"""
    rng = np.random.default_rng(911)
    cost, passable, goal = SO.random_maps(911, 1, 9, 11)
    cost, passable, goal = cost[0], passable[0], goal[0]
    cost[rng.random((9, 11)) < 0.2] = 0
    y, x = np.argwhere(passable == 0)[3]
    goal[y, x] = 1
    assert goal.sum() == 2 and (cost == 0).any()
    return cost, passable, goal


@pytest.mark.parametrize("mask", [HO.MOORE8, HO.VON_NEUMANN, SO.DIRECTED])
@pytest.mark.parametrize("tau", [1.0, 0.05])
def test_oracle_is_logsumexp_and_its_adjoint_is_autograd(mask, tau):
    cost, passable, goal = _issue_map()
    K = 14
    c = torch.from_numpy(cost.astype(f64)).requires_grad_(True)
    V = _torch_field(c, goal, passable, tau, K, mask)
    ref = SO.soft_field(cost, goal, passable, tau, K, mask)
    fin = np.isfinite(ref.dist)
    assert ref.status == 0 and np.array_equal(fin, torch.isfinite(V).numpy()) and fin.sum() > goal.sum() and not fin.all()
    assert ref.dist[goal != 0].tolist() == [0, 0] and np.isinf(ref.dist[(passable == 0) & (goal == 0)]).all()
    scale = np.abs(ref.dist[fin]).max()
    assert np.abs(ref.dist[fin] - V.detach().numpy()[fin]).max() <= 1e-13 * scale
    live = fin & (goal == 0)
    G = np.random.default_rng(5).standard_normal(cost.shape)
    (V[torch.from_numpy(live)] * torch.from_numpy(G[live])).sum().backward()
    G[~live] = np.nan                                            # what is not live is never read
    got = SO.soft_field_grad(cost, goal, passable, G, tau, K, mask)
    assert np.array_equal(got.live, live) and not got.grad[~got.ever].any()
    assert np.abs(got.grad - c.grad.numpy()).max() <= 1e-12 * np.abs(c.grad.numpy()).max()
    # the policy: a distribution on live cells, zeros elsewhere
    rows = ref.policy.sum(0)
    assert np.abs(rows[live] - 1).max() <= 1e-14 and not ref.policy[:, ~live].any()


# ---- 5: against the exact field --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,mask", [(9, 11, HO.MOORE8), (17, 19, HO.VON_NEUMANN), (12, 13, SO.DIRECTED), (32, 33, HO.MOORE8)])
@pytest.mark.parametrize("tau", [0.02, 1.0])
def test_sandwich_between_the_exact_field_and_its_entropy_bound(H, W, mask, tau):
    cost, passable, goal = (a[0] for a in SO.random_maps(H * 31 + W, 1, H, W))
    K = SO.default_horizon(H, W)
    D = FO.field(cost, goal, passable, mask)[0].astype(f64)
    route_hops = GO.field_grad(cost, goal, passable, np.zeros((H, W), f32), mask).hops   # the moves of the OPTIMAL route
    V = SO.soft_field(cost, goal, passable, tau, K, mask).dist
    within = np.isfinite(D) & (route_hops <= K)
    assert within.sum() > 4 and np.isfinite(V[within]).all()
    slack = K * 2.0 ** -23 * D[within].max()                    # D is a float32 sum of at most K terms
    assert (V[within] <= D[within] + slack).all()
    assert (V[within] >= D[within] - K * tau * math.log(len(HO.offsets(mask))) - slack).all()
    if tau == 0.02:
        assert np.abs(V[within] - D[within]).max() <= 0.05 * D[within].max()            # soft is nearly hard


@pytest.mark.parametrize("mask", [HO.MOORE8, HO.VON_NEUMANN, SO.DIRECTED])
def test_infinite_exactly_where_no_goal_lies_within_the_horizon(mask):
    H, W = 11, 14
    cost, passable, goal = (a[0] for a in SO.random_maps(77, 1, H, W))
    hops = SO.hops(goal, passable, mask)
    far = hops.max()
    assert far >= 4
    for K in (1, 3, far - 1, far, SO.default_horizon(H, W)):
        V = SO.soft_field(cost, goal, passable, 0.3, K, mask).dist
        assert np.array_equal(np.isfinite(V), (hops >= 0) & (hops <= K)), K
    V = SO.soft_field(cost, goal, passable, 0.3, far - 1, mask)
    assert np.isinf(V.dist[hops == far]).all() and np.isfinite(V.dist[hops == far - 1]).all()
    none = SO.soft_field(cost, np.zeros_like(goal), passable, 0.3, 8, mask)
    assert none.status == SO.STATUS_NO_GOAL and np.isinf(none.dist).all() and not none.policy.any()
    bad = cost.copy()
    bad[tuple(np.argwhere(passable != 0)[2])] = np.nan
    bad = SO.soft_field(bad, goal, passable, 0.3, 8, mask)
    assert bad.status == SO.STATUS_BAD_COST and np.isinf(bad.dist).all()


# ---- 6: the likelihood of a demonstration; the float32 restatement --------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", [0.02, 0.3, 1.0])
def test_negative_log_likelihood_of_an_optimal_demonstration_is_not_negative(tau):
    H, W = 17, 19
    cost, passable, goal = (a[0] for a in SO.random_maps(4, 1, H, W))
    D = FO.field(cost, goal, passable)[0]
    starts = np.flatnonzero(np.isfinite(D).reshape(-1) & (goal.reshape(-1) == 0))
    K = SO.default_horizon(H, W)
    V = SO.soft_field(cost, goal, passable, tau, K).dist
    for n0 in starts[:: max(1, len(starts) // 6)]:
        path = PO.path(cost, goal, passable, int(n0))
        assert path.status == 0 and len(path.cells) - 1 <= K
        demo = float((cost.astype(f64) * path.mask * (1 - goal)).sum())
        nll = (demo - V.reshape(-1)[n0]) / tau
        assert nll >= -1e-12 * demo / tau
        # its gradient: the demonstration minus the expected visits, which leave the start once at least
        onehot = np.zeros(H * W)
        onehot[n0] = 1
        visits = SO.soft_field_grad(cost, goal, passable, onehot.reshape(H, W), tau, K).grad
        assert visits.reshape(-1)[n0] >= 1 - 1e-12 and visits.sum() >= SO.hops(goal, passable).reshape(-1)[n0] - 1e-9 and (visits >= 0).all()


def test_float32_restatement_stays_inside_the_committed_bounds():
    """the float32 restatement of the recursion and of its adjoint against float64, on the cases of the GPU tests: the scale the kernels'
    error is measured against (tests/soft_fields_oracle.py FWD_RTOL, BWD_RTOL)"""
    worst_f = worst_b = 0.0
    for H, W, B, seed in SO.SHAPE_CASES:
        if H * W > 32 * 33:
            continue
        cost, passable, goal = SO.random_maps(seed, B, H, W)
        for K, tau, mask in SO.sweep_cases(goal[0], passable[0]):
            a = SO.soft_field(cost[0], goal[0], passable[0], tau, K, mask)
            b = SO.soft_field(cost[0], goal[0], passable[0], tau, K, mask, f32)
            fin = np.isfinite(a.dist)
            assert np.array_equal(fin, np.isfinite(b.dist))
            worst_f = max(worst_f, SO.rel_err(b.dist, a.dist))
            G = np.random.default_rng(seed).standard_normal((H, W))
            ga = SO.soft_field_grad(cost[0], goal[0], passable[0], G, tau, K, mask)
            gb = SO.soft_field_grad(cost[0], goal[0], passable[0], G, tau, K, mask, f32)
            worst_b = max(worst_b, SO.rel_err(gb.grad, ga.grad))
    print(f"float32 restatement: forward {worst_f:.3e}, backward {worst_b:.3e}")
    assert 0 < worst_f <= SO.FWD_RTOL and 0 < worst_b <= SO.BWD_RTOL


# ---- 7: Python refusals before a launch; the planner methods ----------------------------------------------------------------------------------------
def test_refusals_before_a_launch_and_the_planner_methods():
    from neural_astar import ops
    from neural_astar.planner import NeuralAstar, VanillaAstar
    from neural_astar.planner.differentiable_astar import DifferentiableAstar
    assert list(inspect.signature(ops.soft_cost_to_go).parameters) == ["cost_maps", "goal_maps", "obstacles_maps", "tau", "horizon", "neighbor_mask",
                                                                       "policies", "differentiable"]
    assert list(inspect.signature(ops.maxent_path_nll).parameters) == ["cost_maps", "start_maps", "goal_maps", "obstacles_maps", "opt_trajs", "tau",
                                                                       "horizon", "neighbor_mask"]
    for cls in (DifferentiableAstar, VanillaAstar, NeuralAstar):
        prm = inspect.signature(cls.soft_cost_to_go).parameters
        assert prm["differentiable"].default is False and prm["policies"].default is False and prm["horizon"].default is None, cls
    assert hasattr(NeuralAstar, "maxent_path_nll")
    m = torch.ones(2, 1, 8, 8, requires_grad=True)
    for tau in (0.0, -0.5, float("nan"), float("inf"), True, None, torch.tensor(1.0)):
        with pytest.raises(ValueError, match="tau"):
            ops.soft_cost_to_go(m, m, m, tau)
        with pytest.raises(ValueError, match="tau"):
            ops.maxent_path_nll(m, m, m, m, m, tau)
    for horizon in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="horizon"):
            ops.soft_cost_to_go(m, m, m, 0.5, horizon=horizon)
    with pytest.raises(ValueError, match="neighbor_mask"):
        ops.soft_cost_to_go(m, m, m, 0.5, neighbor_mask=0x1FF)
    with pytest.raises(ValueError, match="share one"):
        ops.soft_cost_to_go(m, torch.ones(2, 1, 8, 9), m, 0.5)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.soft_cost_to_go(m, m, m, 0.5, differentiable=True)
    big = torch.ones(1, 1, 64, 97)                                # above the backward's limit, below the forward's
    with pytest.raises(NotImplementedError, match="6144"):
        ops.soft_cost_to_go(big, big, big, 0.5, differentiable=True)
    with pytest.raises(RuntimeError, match="HIP device"):         # ... the evaluation call takes it
        ops.soft_cost_to_go(big, big, big, 0.5)
    huge = torch.ones(1, 1, 97, 128)
    with pytest.raises(NotImplementedError, match="12288"):
        ops.soft_cost_to_go(huge, huge, huge, 0.5)
    with pytest.raises(NotImplementedError, match="6144"):
        ops.soft_fields_backward(big, big, big, torch.zeros(8, dtype=torch.uint8), big, 0.5)
    with pytest.raises(ValueError, match="tau"):
        VanillaAstar().soft_cost_to_go(m, m, 0.0)
    with pytest.raises(ValueError, match="tau"):
        NeuralAstar().maxent_path_nll(m, m, m, m, -1.0)
    with pytest.raises(RuntimeError, match="HIP device"):
        DifferentiableAstar().soft_cost_to_go(m, m, m, 0.5)


# ---- 8: the public signatures of the soft family, ops and planners: what callers, probes and the planners' pass-through rely on -----------------
OPS_SIGNATURES = {
    "soft_fields_forward":
        "(cost_maps: 'torch.Tensor', goal_maps: 'torch.Tensor', obstacles_maps: 'torch.Tensor', tau: 'float', horizon: "
        "'Optional[int]' = None, neighbor_mask: 'Optional[int]' = None, policies: 'bool' = False, tape: 'bool' = False)",
    "soft_fields_backward":
        "(cost_maps: 'torch.Tensor', goal_maps: 'torch.Tensor', obstacles_maps: 'torch.Tensor', tape: 'torch.Tensor', "
        "grad_dists: 'torch.Tensor', tau: 'float', horizon: 'Optional[int]' = None, neighbor_mask: 'Optional[int]' = None) -> "
        "'Tuple[torch.Tensor, torch.Tensor]'",
    "soft_fields_tiled_forward":
        "(cost_maps: 'torch.Tensor', goal_maps: 'torch.Tensor', obstacles_maps: 'torch.Tensor', tau: 'float', horizon: "
        "'Optional[int]' = None, neighbor_mask: 'Optional[int]' = None, policies: 'bool' = False, tape: 'bool' = False, "
        "checkpoint_every: 'Optional[int]' = None, sweeps_per_launch: 'Optional[int]' = None)",
    "soft_fields_tiled_backward":
        "(cost_maps: 'torch.Tensor', goal_maps: 'torch.Tensor', obstacles_maps: 'torch.Tensor', tape: 'torch.Tensor', "
        "grad_dists: 'torch.Tensor', tau: 'float', horizon: 'Optional[int]' = None, neighbor_mask: 'Optional[int]' = None, "
        "checkpoint_every: 'Optional[int]' = None) -> 'Tuple[torch.Tensor, torch.Tensor]'",
    "soft_policy_forward":
        "(cost_maps: 'torch.Tensor', goal_maps: 'torch.Tensor', obstacles_maps: 'torch.Tensor', tau: 'float', horizon: "
        "'Optional[int]' = None, neighbor_mask: 'Optional[int]' = None, policies: 'bool' = True, tape: 'bool' = False)",
    "soft_policy_backward":
        "(cost_maps: 'torch.Tensor', goal_maps: 'torch.Tensor', obstacles_maps: 'torch.Tensor', tape: 'torch.Tensor', "
        "grad_dists: 'Optional[torch.Tensor]', grad_log_policies: 'Optional[torch.Tensor]', tau: 'float', horizon: "
        "'Optional[int]' = None, neighbor_mask: 'Optional[int]' = None) -> 'Tuple[torch.Tensor, torch.Tensor]'",
    "soft_policy_tiled_forward":
        "(cost_maps: 'torch.Tensor', goal_maps: 'torch.Tensor', obstacles_maps: 'torch.Tensor', tau: 'float', horizon: "
        "'Optional[int]' = None, neighbor_mask: 'Optional[int]' = None, policies: 'bool' = True, tape: 'bool' = False, "
        "checkpoint_every: 'Optional[int]' = None, sweeps_per_launch: 'Optional[int]' = None)",
    "soft_policy_tiled_backward":
        "(cost_maps: 'torch.Tensor', goal_maps: 'torch.Tensor', obstacles_maps: 'torch.Tensor', tape: 'torch.Tensor', "
        "grad_dists: 'Optional[torch.Tensor]', grad_log_policies: 'Optional[torch.Tensor]', tau: 'float', horizon: "
        "'Optional[int]' = None, neighbor_mask: 'Optional[int]' = None, checkpoint_every: 'Optional[int]' = None) -> "
        "'Tuple[torch.Tensor, torch.Tensor]'",
    "soft_cost_to_go":
        "(cost_maps: 'torch.Tensor', goal_maps: 'torch.Tensor', obstacles_maps: 'torch.Tensor', tau: 'float', horizon: "
        "'Optional[int]' = None, neighbor_mask: 'Optional[int]' = None, policies: 'bool' = False, differentiable: 'bool' = "
        "False) -> 'SoftFieldOutput'",
    "soft_cost_to_go_tiled":
        "(cost_maps: 'torch.Tensor', goal_maps: 'torch.Tensor', obstacles_maps: 'torch.Tensor', tau: 'float', horizon: "
        "'Optional[int]' = None, neighbor_mask: 'Optional[int]' = None, policies: 'bool' = False, differentiable: 'bool' = "
        "False, checkpoint_every: 'Optional[int]' = None) -> 'SoftFieldOutput'",
    "soft_policy":
        "(cost_maps: 'torch.Tensor', goal_maps: 'torch.Tensor', obstacles_maps: 'torch.Tensor', tau: 'float', horizon: "
        "'Optional[int]' = None, neighbor_mask: 'Optional[int]' = None) -> 'SoftPolicyOutput'",
    "soft_policy_tiled":
        "(cost_maps: 'torch.Tensor', goal_maps: 'torch.Tensor', obstacles_maps: 'torch.Tensor', tau: 'float', horizon: "
        "'Optional[int]' = None, neighbor_mask: 'Optional[int]' = None, checkpoint_every: 'Optional[int]' = None) -> "
        "'SoftPolicyOutput'",
    "maxent_path_nll":
        "(cost_maps: 'torch.Tensor', start_maps: 'torch.Tensor', goal_maps: 'torch.Tensor', obstacles_maps: 'torch.Tensor', "
        "opt_trajs: 'torch.Tensor', tau: 'float', horizon: 'Optional[int]' = None, neighbor_mask: 'Optional[int]' = None) -> "
        "'torch.Tensor'",
    "maxent_path_nll_tiled":
        "(cost_maps: 'torch.Tensor', start_maps: 'torch.Tensor', goal_maps: 'torch.Tensor', obstacles_maps: 'torch.Tensor', "
        "opt_trajs: 'torch.Tensor', tau: 'float', horizon: 'Optional[int]' = None, neighbor_mask: 'Optional[int]' = None, "
        "checkpoint_every: 'Optional[int]' = None) -> 'torch.Tensor'",
    "soft_policy_nll":
        "(cost_maps: 'torch.Tensor', goal_maps: 'torch.Tensor', obstacles_maps: 'torch.Tensor', opt_policies: 'torch.Tensor', "
        "tau: 'float', horizon: 'Optional[int]' = None, neighbor_mask: 'Optional[int]' = None) -> 'torch.Tensor'",
    "soft_policy_nll_tiled":
        "(cost_maps: 'torch.Tensor', goal_maps: 'torch.Tensor', obstacles_maps: 'torch.Tensor', opt_policies: 'torch.Tensor', "
        "tau: 'float', horizon: 'Optional[int]' = None, neighbor_mask: 'Optional[int]' = None, checkpoint_every: "
        "'Optional[int]' = None) -> 'torch.Tensor'",
}
PLANNER_SIGNATURES = {
    ("DifferentiableAstar", "soft_cost_to_go"):
        "(self, cost_maps: 'torch.Tensor', goal_maps: 'torch.Tensor', obstacles_maps: 'torch.Tensor', tau: 'float', horizon: "
        "'Optional[int]' = None, policies: 'bool' = False, differentiable: 'bool' = False) -> " '"\'ops.SoftFieldOutput\'"',
    ("DifferentiableAstar", "soft_cost_to_go_tiled"):
        "(self, cost_maps: 'torch.Tensor', goal_maps: 'torch.Tensor', obstacles_maps: 'torch.Tensor', tau: 'float', horizon: "
        "'Optional[int]' = None, policies: 'bool' = False, differentiable: 'bool' = False, checkpoint_every: 'Optional[int]' = "
        "None) -> " '"\'ops.SoftFieldOutput\'"',
    ("DifferentiableAstar", "maxent_path_nll"):
        "(self, cost_maps: 'torch.Tensor', start_maps: 'torch.Tensor', goal_maps: 'torch.Tensor', obstacles_maps: "
        "'torch.Tensor', opt_trajs: 'torch.Tensor', tau: 'float', horizon: 'Optional[int]' = None, tiled: 'bool' = False, "
        "checkpoint_every: 'Optional[int]' = None) -> 'torch.Tensor'",
    ("DifferentiableAstar", "soft_policy"):
        "(self, cost_maps: 'torch.Tensor', goal_maps: 'torch.Tensor', obstacles_maps: 'torch.Tensor', tau: 'float', horizon: "
        "'Optional[int]' = None) -> " '"\'ops.SoftPolicyOutput\'"',
    ("DifferentiableAstar", "soft_policy_tiled"):
        "(self, cost_maps: 'torch.Tensor', goal_maps: 'torch.Tensor', obstacles_maps: 'torch.Tensor', tau: 'float', horizon: "
        "'Optional[int]' = None, checkpoint_every: 'Optional[int]' = None) -> " '"\'ops.SoftPolicyOutput\'"',
    ("DifferentiableAstar", "policy_nll"):
        "(self, cost_maps: 'torch.Tensor', goal_maps: 'torch.Tensor', obstacles_maps: 'torch.Tensor', opt_policies: "
        "'torch.Tensor', tau: 'float', horizon: 'Optional[int]' = None, tiled: 'bool' = False, checkpoint_every: "
        "'Optional[int]' = None) -> 'torch.Tensor'",
    ("VanillaAstar", "soft_cost_to_go"):
        "(self, map_designs: 'torch.Tensor', goal_maps: 'torch.Tensor', tau: 'float', horizon: 'Optional[int]' = None, "
        "policies: 'bool' = False, differentiable: 'bool' = False)",
    ("VanillaAstar", "soft_cost_to_go_tiled"):
        "(self, map_designs: 'torch.Tensor', goal_maps: 'torch.Tensor', tau: 'float', horizon: 'Optional[int]' = None, "
        "policies: 'bool' = False, differentiable: 'bool' = False, checkpoint_every: 'Optional[int]' = None)",
    ("VanillaAstar", "maxent_path_nll"):
        "(self, map_designs: 'torch.Tensor', start_maps: 'torch.Tensor', goal_maps: 'torch.Tensor', opt_trajs: 'torch.Tensor', "
        "tau: 'float', horizon: 'Optional[int]' = None, tiled: 'bool' = False, checkpoint_every: 'Optional[int]' = None) -> "
        "'torch.Tensor'",
    ("VanillaAstar", "soft_policy"):
        "(self, map_designs: 'torch.Tensor', goal_maps: 'torch.Tensor', tau: 'float', horizon: 'Optional[int]' = None)",
    ("VanillaAstar", "soft_policy_tiled"):
        "(self, map_designs: 'torch.Tensor', goal_maps: 'torch.Tensor', tau: 'float', horizon: 'Optional[int]' = None, "
        "checkpoint_every: 'Optional[int]' = None)",
    ("VanillaAstar", "policy_nll"):
        "(self, map_designs: 'torch.Tensor', goal_maps: 'torch.Tensor', opt_policies: 'torch.Tensor', tau: 'float', horizon: "
        "'Optional[int]' = None, tiled: 'bool' = False, checkpoint_every: 'Optional[int]' = None) -> 'torch.Tensor'",
    ("NeuralAstar", "soft_cost_to_go"):
        "(self, map_designs: 'torch.Tensor', start_maps: 'torch.Tensor', goal_maps: 'torch.Tensor', tau: 'float', horizon: "
        "'Optional[int]' = None, policies: 'bool' = False, differentiable: 'bool' = False)",
    ("NeuralAstar", "soft_cost_to_go_tiled"):
        "(self, map_designs: 'torch.Tensor', start_maps: 'torch.Tensor', goal_maps: 'torch.Tensor', tau: 'float', horizon: "
        "'Optional[int]' = None, policies: 'bool' = False, differentiable: 'bool' = False, checkpoint_every: 'Optional[int]' = "
        'None)',
    ("NeuralAstar", "maxent_path_nll"):
        "(self, map_designs: 'torch.Tensor', start_maps: 'torch.Tensor', goal_maps: 'torch.Tensor', opt_trajs: 'torch.Tensor', "
        "tau: 'float', horizon: 'Optional[int]' = None, tiled: 'bool' = False, checkpoint_every: 'Optional[int]' = None) -> "
        "'torch.Tensor'",
    ("NeuralAstar", "soft_policy"):
        "(self, map_designs: 'torch.Tensor', start_maps: 'torch.Tensor', goal_maps: 'torch.Tensor', tau: 'float', horizon: "
        "'Optional[int]' = None)",
    ("NeuralAstar", "soft_policy_tiled"):
        "(self, map_designs: 'torch.Tensor', start_maps: 'torch.Tensor', goal_maps: 'torch.Tensor', tau: 'float', horizon: "
        "'Optional[int]' = None, checkpoint_every: 'Optional[int]' = None)",
    ("NeuralAstar", "policy_nll"):
        "(self, map_designs: 'torch.Tensor', start_maps: 'torch.Tensor', goal_maps: 'torch.Tensor', opt_policies: "
        "'torch.Tensor', tau: 'float', horizon: 'Optional[int]' = None, tiled: 'bool' = False, checkpoint_every: "
        "'Optional[int]' = None) -> 'torch.Tensor'",
}


def test_soft_family_public_signatures_are_frozen():
    from neural_astar import ops, planner
    from neural_astar.planner.differentiable_astar import DifferentiableAstar
    assert len(OPS_SIGNATURES) == 16 and set(OPS_SIGNATURES) <= set(ops.__all__)
    for name, signature in OPS_SIGNATURES.items():
        assert str(inspect.signature(getattr(ops, name))) == signature, name
    classes = {"DifferentiableAstar": DifferentiableAstar, "VanillaAstar": planner.VanillaAstar, "NeuralAstar": planner.NeuralAstar}
    assert len(PLANNER_SIGNATURES) == 18
    for (cls, name), signature in PLANNER_SIGNATURES.items():
        assert str(inspect.signature(getattr(classes[cls], name))) == signature, (cls, name)
