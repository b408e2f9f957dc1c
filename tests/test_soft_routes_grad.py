"""CPU: the score-function backward of the sampled routes (include/nastar_soft_routes_grad.h, ``ops.soft_routes(..., differentiable=True)``,
``ops.soft_routes_backward``, ``ops.route_score_loss``) -- everything that needs no GPU.

1. the twentieth header against ``_native.SOFT_ROUTES_GRAD_SIGNATURES``; the library exports the four symbols; every refusal the entry
   point makes before any HIP call, and their order;
2. ``route_score_loss`` on hand-made tensors: a failed query, the per-query baseline, an all-failed batch;
3. the fixed point of tests/soft_routes_grad_oracle.py against float64 on the float64 walker's routes;
4. the Python refusals made before a launch, and the planner methods.
"""
import inspect

import numpy as np
import pytest
import torch

import soft_fields_oracle as SO
import soft_routes_grad_oracle as GO
import soft_routes_oracle as RO
from test_fields import _defines, _prototypes

f32, f64 = np.float32, np.float64
NAMES = ["nastar_soft_routes_backward", "nastar_soft_routes_grad_abi", "nastar_soft_routes_grad_max_cells", "nastar_soft_routes_grad_workspace_bytes"]
ARGS = ["cost", "goal", "passable", "tape", "tape_bytes", "start_idx", "routes", "route_cap", "route_len", "status", "grad_log_prob", "B", "S",
        "N", "H", "W", "neighbor_mask", "tau", "horizon", "grad_cost_out", "status_out", "workspace", "workspace_bytes", "stream"]


# ---- 1: header, binding, library, refusals ----------------------------------------------------------------------------------------------------
def test_twentieth_header_and_its_signature_table_agree():
    from neural_astar import _native
    protos = _prototypes("nastar_soft_routes_grad.h")
    assert sorted(protos) == sorted(_native.SOFT_ROUTES_GRAD_SIGNATURES) == NAMES
    for name, (ret, args) in protos.items():
        assert _native.SOFT_ROUTES_GRAD_SIGNATURES[name] == ret + " " + "".join(k for k, _ in args), name
    assert [n for _, n in protos["nastar_soft_routes_backward"][1]] == ARGS
    assert [n for _, n in protos["nastar_soft_routes_grad_workspace_bytes"][1]] == ["B", "H", "W"]
    # a table of its own: the other tables and headers are what they were
    for table in (_native.SIGNATURES, _native.SOFT_FIELD_SIGNATURES, _native.SOFT_ROUTE_SIGNATURES, _native.SOFT_ROUTES_TILED_SIGNATURES):
        assert not set(_native.SOFT_ROUTES_GRAD_SIGNATURES) & set(table)
    assert len(_native.SIGNATURES) == 74 and len(_native.SOFT_ROUTE_SIGNATURES) == 4 == len(_prototypes("nastar_soft_routes.h"))
    assert _defines("nastar_soft_routes_grad.h") == {"NASTAR_SOFT_ROUTES_GRAD_ABI": 1} and _defines("nastar.h")["NASTAR_VERSION"] == 800


def test_library_exports_the_four_symbols():
    from neural_astar import _native, ops
    lib = _native.load()
    for sym in NAMES:
        assert hasattr(lib, sym), sym
    assert lib.nastar_soft_routes_grad_abi() == 1
    assert lib.nastar_soft_routes_grad_max_cells() == lib.nastar_soft_fields_grad_max_cells() == 6144 == ops.SOFT_ROUTES_GRAD_MAX_CELLS
    assert len(lib.nastar_soft_routes_backward.argtypes) == 24
    # two int64 and two fp32 planes and 8 bytes of scale per map, in whole 16 bytes
    assert lib.nastar_soft_routes_grad_workspace_bytes(2, 8, 8) == 2 * 64 * 24 + 16
    assert lib.nastar_soft_routes_grad_workspace_bytes(3, 5, 7) == (3 * 35 * 24 + 24 + 15) // 16 * 16
    assert lib.nastar_soft_routes_grad_workspace_bytes(0, 8, 8) == 0 == lib.nastar_soft_routes_grad_workspace_bytes(1, 8, -1)
    assert {"soft_routes_backward", "route_score_loss", "SOFT_ROUTES_GRAD_MAX_CELLS"} <= set(ops.__all__)


P = 0x10000  # never dereferenced: every call below is refused on its arguments
WS = 2 * 64 * 24 + 16


def _call(**over):
    a = dict(cost=P, goal=P, passable=P, tape=P, tape_bytes=2 * 64 * 16 * 4, start_idx=P, routes=P, route_cap=17, route_len=P, status=P,
             grad_log_prob=P, B=2, S=3, N=5, H=8, W=8, neighbor_mask=0x1EF, tau=0.5, horizon=16, grad_cost_out=P, status_out=P, workspace=P,
             workspace_bytes=WS, stream=None)
    a.update(over)
    return a


@pytest.mark.parametrize("over,rc", [
    (dict(neighbor_mask=0x1FF), 2), (dict(neighbor_mask=0x200), 2),
    (dict(cost=None), 5), (dict(goal=None), 5), (dict(passable=None), 5), (dict(tape=None), 5), (dict(start_idx=None), 5), (dict(routes=None), 5),
    (dict(route_len=None), 5), (dict(status=None), 5), (dict(grad_log_prob=None), 5), (dict(grad_cost_out=None), 5), (dict(status_out=None), 5),
    (dict(B=0), 1), (dict(S=0), 1), (dict(N=-1), 1), (dict(H=0), 1), (dict(W=-1), 1), (dict(horizon=0), 1), (dict(tau=0.0), 1),
    (dict(tau=float("nan")), 1), (dict(tau=float("inf")), 1), (dict(tau=-1.0), 1),
    (dict(route_cap=16), 1), (dict(route_cap=0), 1), (dict(route_cap=-4), 1),      # rows shorter than horizon + 1
    (dict(horizon=2 ** 31 - 1, route_cap=2 ** 31 - 1), 1),                          # (horizon + 1 does not wrap)
    (dict(neighbor_mask=0x010, cost=None), 2),                                      # the mask is looked at first
    (dict(cost=None, B=0), 5),                                                      # a NULL before the shape
    (dict(N=0, H=128, W=129), 1),                                                   # the shape before the limit
    (dict(route_cap=16, H=128, W=129), 1),                                          # the row length before the limit
    (dict(H=1, W=6145), 2), (dict(H=64, W=97), 2), (dict(H=65536, W=65536), 2),
    (dict(B=1 << 10, S=1 << 10, N=(1 << 10) + 1), 2),                              # more than 2^30 walkers
    (dict(S=1 << 30, N=1 << 30), 2),
    (dict(B=1, S=1 << 14, N=1 << 14, horizon=16, tape_bytes=0), 2),                # S * N * K = 2^32: P = 29, before the tape
    (dict(H=1, W=6145, tape_bytes=0, workspace_bytes=0), 2),                        # the limit before the tape and the workspace
    (dict(tape_bytes=2 * 64 * 16 * 4 - 1), 6), (dict(tape=P + 8), 6), (dict(horizon=17, route_cap=18), 6), (dict(B=3), 6),
    (dict(workspace=None), 6), (dict(workspace_bytes=WS - 1), 6), (dict(workspace=P + 8), 6), (dict(workspace_bytes=0), 6)])
def test_soft_routes_backward_refuses_bad_arguments_without_a_device(over, rc):
    from neural_astar import _native
    lib = _native.load()
    assert lib.nastar_soft_routes_backward(*_call(**over).values()) == rc
    assert lib.nastar_last_error() == b""


def test_the_bits_rule_is_the_headers():
    from neural_astar import _native
    lib = _native.load()
    # S * N * K = 2^31 leaves P = 30 and passes the rule (the tape is then what is wrong); one more walker leaves 29
    assert GO.bits(1 << 13, 1 << 14, 16) == 30 and GO.bits((1 << 13) + 1, 1 << 14, 16) == 29
    assert lib.nastar_soft_routes_backward(*_call(B=1, S=1 << 13, N=1 << 14, tape_bytes=0).values()) == 6
    assert lib.nastar_soft_routes_backward(*_call(B=1, S=(1 << 13) + 1, N=1 << 14, tape_bytes=0).values()) == 2
    assert GO.bits(1, 1, 1) == 40 == GO.bits(4, 75, 2 ** 21 // 300) and GO.bits(1, 1, (1 << 21) + 1) == 39
    # P is 40 at every shape the GPU tests run
    for H, W, B, seed in GO.SHAPE_CASES:
        for K, tau, mask, (S, N), _ in GO.cases(H, W, B, seed):
            assert GO.bits(S, N, K) == 40, (H, W, K, S, N)
    assert GO.bits(1, 16384, 24) == 40 and GO.bits(4, 75, 16) == 40


# ---- 2: route_score_loss ------------------------------------------------------------------------------------------------------------------------
def test_route_score_loss_masks_failed_queries_and_centres_per_query():
    from neural_astar import ops
    inf = float("inf")
    logp = torch.tensor([[[-1.0, -2.0, -3.0], [-inf, -inf, -inf]],
                         [[-0.5, -0.25, -4.0], [-1.5, -2.5, -3.5]]], requires_grad=True)
    rewards = torch.tensor([[[1.0, 2.0, 6.0], [inf, inf, inf]],
                            [[10.0, 20.0, 30.0], [5.0, 5.0, 8.0]]])
    status = torch.tensor([[0, 3], [0, 0]], dtype=torch.int32)
    loss = ops.route_score_loss(logp, rewards, status)
    # baseline "mean" is per query: 3, -, 20, 6
    adv = torch.tensor([[[-2.0, -1.0, 3.0], [0, 0, 0]], [[-10.0, 0.0, 10.0], [-1.0, -1.0, 2.0]]])
    lp = torch.where(torch.isfinite(logp.detach()), logp.detach(), torch.zeros(()))
    assert torch.isfinite(loss) and torch.allclose(loss, (adv * lp).sum() / 9)
    loss.backward()
    assert torch.isfinite(logp.grad).all() and torch.equal(logp.grad[0, 1], torch.zeros(3)) and torch.allclose(logp.grad, adv / 9)
    # no baseline, and a tensor
    assert torch.allclose(ops.route_score_loss(logp.detach(), rewards, status, baseline=None),
                          (torch.where(torch.isfinite(rewards), rewards, torch.zeros(())) * lp).sum() / 9)
    b = torch.tensor([[[1.0], [0.0]], [[2.0], [3.0]]])
    ok = torch.tensor([[[True], [False]], [[True], [True]]])
    want = (torch.where(ok, rewards - b, torch.zeros(())) * lp).sum() / 9
    assert torch.allclose(ops.route_score_loss(logp.detach(), rewards, status, baseline=b), want)
    # integer rewards (route_lengths) are taken as they are
    lens = torch.tensor([[[2, 3, 7], [0, 0, 0]], [[1, 1, 1], [4, 5, 6]]], dtype=torch.int32)
    assert torch.allclose(ops.route_score_loss(logp.detach(), lens, status, None), (lens.float() * lp).sum() / 9)
    # the product with 0 this helper exists to avoid
    assert torch.isnan((torch.zeros(3) * logp.detach()[0, 1]).sum())


def test_route_score_loss_of_an_all_failed_batch_is_zero():
    from neural_astar import ops
    logp = torch.full((2, 2, 4), -float("inf"), requires_grad=True)
    rewards = torch.full((2, 2, 4), float("inf"))
    status = torch.tensor([[1, 3], [9, 9]], dtype=torch.int32)
    for baseline in ("mean", None, torch.zeros(2, 2, 1)):
        loss = ops.route_score_loss(logp, rewards, status, baseline)
        assert loss.item() == 0.0
        g, = torch.autograd.grad(loss, logp)
        assert torch.equal(g, torch.zeros_like(g))
    with pytest.raises(ValueError, match="baseline"):
        ops.route_score_loss(logp, rewards, status, baseline="median")
    with pytest.raises(ValueError, match="rewards"):
        ops.route_score_loss(logp, rewards[:, :1], status)
    with pytest.raises(ValueError, match="status"):
        ops.route_score_loss(logp, rewards, status[:1])


# ---- 3: the fixed point against float64 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,B,seed", [(1, 9, 1, 2), (5, 7, 3, 4), (16, 16, 2, 7)], ids=lambda v: str(v))
def test_fixed_point_sums_against_float64_on_the_walkers_routes(H, W, B, seed):
    cost, passable, goal = RO.case_maps(H, W, B, seed)
    HW = H * W
    worst = 0.0
    for K, tau, mask, (S, N), sample_seed in GO.cases(H, W, B, seed):
        starts = RO.case_starts(sample_seed, S, passable, goal)
        g = np.random.default_rng(sample_seed).standard_normal((B, S, N)).astype(f32)
        g[..., ::2] *= f32(2.0 ** -30)   # (a float32 within 2^-16 of M_b is a whole number of units: small weights make the rounding show)
        uni = RO.case_uniforms(sample_seed, B, S, N)
        routes, lengths, status = [], [], []
        for b in range(B):
            fld = SO.soft_field(cost[b], goal[b], passable[b], tau, K, mask)
            sel = slice(b * S * N, (b + 1) * S * N)
            r = RO.walk(fld.planes, cost[b], goal[b], passable[b], np.repeat(starts[b], N), tau, mask, lambda j, sel=sel: uni(j)[sel])
            routes.append(RO.padded(r.cells, K + 1).reshape(S, N, K + 1))
            lengths.append(np.array([len(c) for c in r.cells]).reshape(S, N))
            status.append(r.status.reshape(S, N)[:, 0])
        status = np.stack(status)
        q, e, P, kind = GO.quantise(g, status == 0, S, N, K)
        assert P == 40
        for b in range(B):
            if kind[b] != GO.NORMAL:
                assert not (status[b] == 0).any()
                continue
            M = np.abs(g[b][status[b] == 0]).max().astype(f64)
            assert 2.0 ** e[b] <= M < 2.0 ** (e[b] + 1) and np.abs(q[b]).max() <= 2 ** (P + 1)
            qv, qs = GO.q_planes(routes[b], lengths[b], starts[b], q[b], HW)
            ref, count = GO.weighted_visits(routes[b], lengths[b], status[b], g[b], HW)
            err = np.abs(np.array([float(v) for v in qv]) * 2.0 ** (e[b] - P) - ref)
            assert (err <= 2.0 ** -(P - 1) * M * count).all(), (H, W, K, tau, mask, b)
            seeds = GO.seeds64(starts[b], status[b], g[b], HW)
            per_start = np.zeros(HW)
            for s in range(S):
                if status[b, s] == 0:
                    per_start[starts[b, s]] += N
            assert (np.abs(np.array([float(v) for v in qs]) * 2.0 ** (e[b] - P) - seeds) <= 2.0 ** -(P - 1) * M * per_start).all()
            if count.any():
                worst = max(worst, float((err[count > 0] / (M * count[count > 0])).max()))
    print(f"{B}x{H}x{W}: worst fixed-point error per unit of visit count {worst:.3e} of M_b (bound 2^-39 = {2.0 ** -39:.3e})")


def test_quantise_by_hand():
    ok = np.array([[True, False], [True, True], [False, False], [True, True]])
    g = np.array([[[0.75, -3.0], [np.nan, np.inf]],            # the failed query's NaN is not read: M = 3, e = 1
                  [[0.0, 0.0], [0.0, -0.0]],                   # M = 0
                  [[1.0, 2.0], [3.0, 4.0]],                    # no ok walker
                  [[1.0, np.inf], [2.0, 3.0]]], f32)           # an ok walker's infinity
    q, e, P, kind = GO.quantise(g, ok, 2, 2, 24)
    assert P == 40 and kind == [GO.NORMAL, GO.ZERO, GO.ZERO, GO.NOT_FINITE] and e[0] == 1
    assert q[0].tolist() == [[3 << 37, -(3 << 39)], [0, 0]] and not q[1:].any()
    # exponents: a power of two, just below one, a subnormal
    for M, want in ((4.0, 2), (np.nextafter(f32(4.0), f32(0)), 1), (2.0 ** -149, -149), (1.5 * 2.0 ** -140, -140)):
        q, e, P, kind = GO.quantise(np.array([[[M, M / 2]]], f32), np.array([[True]]), 1, 2, 1)
        assert e == [want] and 2 ** P <= q[0, 0, 0] < 2 ** (P + 1)
    # ties go to even
    q, e, P, _ = GO.quantise(np.array([[[1.0, 2.0 ** -41, 3 * 2.0 ** -41, -(2.0 ** -41)]]], f32), np.array([[True]]), 1, 4, 1)
    assert q[0, 0].tolist() == [2 ** 40, 0, 2, 0]
    assert GO.combine(np.array([1.0, 0.0], f32), [1 << 40, -(1 << 39)], 0, 40, 0.5).tolist() == [0.0, 1.0]
    assert GO.seed_plane([3 << 39, 0], 1, 40).tolist() == [3.0, 0.0]


# ---- 4: the Python side ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_before_a_launch_and_the_planner_methods():
    from neural_astar import ops, planner
    from neural_astar.planner.differentiable_astar import DifferentiableAstar
    m = torch.ones(2, 1, 8, 8, requires_grad=True)
    st = torch.zeros(2, 3, dtype=torch.int64)
    assert str(inspect.signature(ops.soft_routes)).endswith("uniforms: 'Optional[torch.Tensor]' = None, differentiable: 'bool' = False) -> 'SoftRoutes'")
    assert str(inspect.signature(ops.soft_routes_tiled)).endswith("differentiable: 'bool' = False, checkpoint_every: 'Optional[int]' = None) -> 'SoftRoutes'")
    with pytest.raises(TypeError, match="differentiable"):      # (a checkpoint_every passed by position where it used to stand)
        ops.soft_routes_tiled(m, m, m, st, 0.5, None, 1, 1, None, None, False, None, 8)
    with pytest.raises(ValueError, match=r"max_route_len >= horizon \+ 1 = 33"):
        ops.soft_routes(m, m, m, st, 0.5, seed=1, max_route_len=32, differentiable=True)
    with pytest.raises(ValueError, match=r"horizon \+ 1 = 17"):
        ops.soft_routes(m, m, m, st, 0.5, horizon=16, seed=1, max_route_len=16, differentiable=True)
    with pytest.raises(ValueError, match="max_route_len"):      # (the evaluation call's own refusals come first)
        ops.soft_routes(m, m, m, st, 0.5, seed=1, max_route_len=0, differentiable=True)
    with pytest.raises(ValueError, match="tau"):
        ops.soft_routes(m, m, m, st, 0.0, seed=1, differentiable=True)
    big = torch.ones(1, 1, 1, 6145)
    with pytest.raises(NotImplementedError, match="6144.*12288"):
        ops.soft_routes(big, big, big, torch.zeros(1, 1, dtype=torch.int64), 0.5, seed=1, differentiable=True)
    with pytest.raises(NotImplementedError, match="fraction bits"):
        ops.soft_routes(m, m, m, torch.zeros(2, 1 << 13, dtype=torch.int64), 0.5, horizon=16, num_samples=(1 << 14) + 2, seed=1, differentiable=True)
    with pytest.raises(NotImplementedError, match="differentiable=True is not built"):
        ops.soft_routes_tiled(m, m, m, st, 0.5, seed=1, differentiable=True)
    # the raw call
    tape = torch.zeros(16, dtype=torch.uint8)
    rows, lens, status, g = (torch.zeros(2, 3, 5, 33, dtype=torch.int32), torch.zeros(2, 3, 5, dtype=torch.int32),
                             torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, 3, 5))
    with pytest.raises(ValueError, match="routes"):
        ops.soft_routes_backward(m, m, m, tape, st, rows.long(), lens, status, g, 0.5)
    with pytest.raises(ValueError, match=r"horizon \+ 1 = 33"):
        ops.soft_routes_backward(m, m, m, tape, st, rows[..., :32], lens, status, g, 0.5)
    with pytest.raises(ValueError, match="route_lengths"):
        ops.soft_routes_backward(m, m, m, tape, st, rows, lens[:, :2], status, g, 0.5)
    with pytest.raises(ValueError, match="status"):
        ops.soft_routes_backward(m, m, m, tape, st, rows, lens, status.long(), g, 0.5)
    with pytest.raises(ValueError, match="grad_log_probs"):
        ops.soft_routes_backward(m, m, m, tape, st, rows, lens, status, g.double(), 0.5)
    with pytest.raises(NotImplementedError, match="6144.*12288"):
        ops.soft_routes_backward(big, big, big, tape, torch.zeros(1, 1, dtype=torch.int64), torch.zeros(1, 1, 1, 12293, dtype=torch.int32),
                                 torch.zeros(1, 1, 1, dtype=torch.int32), torch.zeros(1, 1, dtype=torch.int32), torch.zeros(1, 1, 1), 0.5)
    # the planners: ``sample_routes`` keeps its signature (tests/test_soft_routes.py pins it); the differentiable call is a method of its
    # own with the same arguments
    want = str(inspect.signature(DifferentiableAstar.sample_routes))
    assert str(inspect.signature(DifferentiableAstar.sample_routes_differentiable)) == want
    for cls in (planner.VanillaAstar, planner.NeuralAstar):
        assert str(inspect.signature(cls.sample_routes_differentiable)) == str(inspect.signature(cls.sample_routes))
    with pytest.raises(NotImplementedError, match="encoder_input"):
        planner.NeuralAstar(encoder_input="m+").sample_routes_differentiable(m, st, m, 0.5)
    na = planner.NeuralAstar(encoder_input="m")
    with pytest.raises(ValueError, match="max_route_len"):
        na.sample_routes_differentiable(m, st, m, 0.5, max_route_len=0)
    with pytest.raises(ValueError, match="tau"):
        na.sample_routes_differentiable(m, st, m, 0.0)
    with pytest.raises(ValueError, match="num_samples"):
        na.sample_routes_differentiable(m, st, m, 0.5, num_samples=0)
