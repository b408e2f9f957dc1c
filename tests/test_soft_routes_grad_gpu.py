"""GPU: the score-function backward of the sampled routes (include/nastar_soft_routes_grad.h, ``ops.soft_routes(..., differentiable=True)``,
``ops.soft_routes_backward``).

1. to the bit: ``log_probs.backward(g)`` against tests/soft_routes_grad_oracle.py's ``expected`` -- the fixed-point sums in Python integers over
   the device's own routes, ``ops.soft_fields_backward`` (the existing kernel) of the oracle's seed plane, the header's store: 0 differing
   elements, no tolerance;
2. against the float64 reference within ``SO.BWD_RTOL`` of the size of the gradient's two terms;
3. the estimator estimates: the REINFORCE gradient of the expected route length against a finite difference of the float64 oracle;
4. a pure function of the inputs;  5. what is not read;  6. the limit;  7. the surface: autograd, the planners, a captured graph.
The figures are printed before they are asserted.
"""
import functools

import numpy as np
import pytest
import torch

import soft_fields_oracle as SO
import soft_routes_grad_oracle as GO
import soft_routes_oracle as RO

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
MOORE8 = SO.MOORE8


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


def _t(a, dtype=f32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(_dev())


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _same(a, b):
    """the number of elements of two float32 arrays whose bits differ"""
    return int((_bits(a) != _bits(b)).sum())


def _forward(c, g, p, tau, K, mask):
    """the tape as ``soft_routes`` writes it"""
    from neural_astar import ops
    return ops.soft_fields_forward(c, g, p, tau, K, neighbor_mask=mask, tape=True)[1]


def _expected(c, g, p, tape, routes, lengths, starts, status, grad, K, tau, mask, map_status=None):
    """``GO.expected`` with the device's field backward: numpy in, [B,H,W] float32 out"""
    from neural_astar import ops
    B, H, W = c.shape

    def field_backward(seed):
        return ops.soft_fields_backward(c, g, p, tape, _t(seed.reshape(B, 1, H, W)), tau, K, mask)[0].cpu().numpy()

    return GO.expected(routes, lengths, starts, status, grad, H * W, K, tau, field_backward, map_status).reshape(B, H, W)


@functools.lru_cache(maxsize=None)
def _case_results(H, W, B, seed):
    """every case of one shape, run ONCE for the bit test and the float64 test -> [(what, (K, tau, mask), starts, g, numpy outputs of the
    differentiable call, grad_cost [B,H,W], expected [B,H,W])]"""
    from neural_astar import ops
    cost, passable, goal = RO.case_maps(H, W, B, seed)
    c, g, p = _t(cost), _t(goal), _t(passable)
    done = []
    for K, tau, mask, (S, N), sample_seed in GO.cases(H, W, B, seed):
        what = f"{B}x{H}x{W} K={K} tau={tau} mask={mask:#05x} S={S} N={N}"
        starts = RO.case_starts(sample_seed, S, passable, goal)
        up = np.random.default_rng(sample_seed).standard_normal((B, S, N)).astype(f32)
        leaf = c.clone().requires_grad_(True)
        out = ops.soft_routes(leaf, g, p, _t(starts, np.int32), tau, K, N, sample_seed, neighbor_mask=mask, differentiable=True)
        assert out.log_probs.requires_grad and tuple(out.routes.shape) == (B, S, N, K + 1), what
        out.log_probs.backward(_t(up))
        got = leaf.grad.cpu().numpy()
        routes, lengths, status = out.routes.cpu().numpy(), out.route_lengths.cpu().numpy(), out.status.cpu().numpy()
        want = _expected(c, g, p, _forward(c, g, p, tau, K, mask), routes, lengths, starts, status, up, K, tau, mask)
        done.append((what, (K, tau, mask), starts, up, (routes, lengths, status), got, want))
    return cost, passable, goal, done


# ---- 1: to the bit ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,B,seed", GO.SHAPE_CASES, ids=lambda v: str(v))
def test_gradient_is_the_definition_to_the_bit(H, W, B, seed):
    _, _, _, done = _case_results(H, W, B, seed)
    assert done
    moved = 0
    for what, _, _, _, _, got, want in done:
        assert got.shape == want.shape and _same(got, want) == 0, (what, _same(got, want))
        moved += int(np.count_nonzero(got))
    assert moved > 0 or H * W == 1   # (the cases do reach the costs)


# ---- 2: against float64 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,B,seed", GO.SHAPE_CASES, ids=lambda v: str(v))
def test_gradient_against_float64(H, W, B, seed):
    cost, passable, goal, done = _case_results(H, W, B, seed)
    worst = 0.0
    for what, (K, tau, mask), starts, up, (routes, lengths, status), got, _ in done:
        for b in range(B):
            ref, scale = GO.reference(cost[b], goal[b], passable[b], routes[b], lengths[b], starts[b], status[b], up[b], tau, K, mask)
            assert np.isfinite(got[b]).all(), what
            err = float(np.abs(got[b].reshape(-1).astype(f64) - ref).max() / scale) if scale > 0 else float(np.abs(got[b]).max())
            worst = max(worst, err)
            assert err <= SO.BWD_RTOL, (what, b, err)
    print(f"{B}x{H}x{W}: worst error against float64 {worst:.3e} of max|A_ref| + max|B_ref| (bound {SO.BWD_RTOL:.3e})")


# ---- 3: the estimator estimates ----------------------------------------------------------------------------------------------------------------------
def test_reinforce_gradient_of_the_expected_length_is_the_finite_difference():
    from neural_astar import ops
    H, W, B, seed = 5, 7, 3, 4
    tau, K, N, chunk = 0.3, SO.default_horizon(5, 7), 16384, 512
    cost, passable, goal = RO.case_maps(H, W, B, seed)
    starts = np.array([[int(np.argmax(SO.hops(goal[b], passable[b]).reshape(-1)))] for b in range(B)], np.int32)   # argmax: the lowest index

    def expected_len(cm, b):   # E[len] = 1 + the expected visits of the cells a route leaves: the oracle's one-hot backward
        G = np.zeros((H, W))
        G.reshape(-1)[starts[b, 0]] = 1
        return 1.0 + SO.soft_field_grad(cm, goal[b], passable[b], G, tau, K, MOORE8).grad.sum()

    leaf = _t(cost).requires_grad_(True)
    out = ops.soft_routes(leaf, _t(goal), _t(passable), _t(starts, np.int32), tau, K, N, 11, differentiable=True)
    assert (out.status == 0).all()
    base = torch.tensor([expected_len(cost[b], b) for b in range(B)], dtype=torch.float64, device=_dev()).view(B, 1, 1)
    adv = (out.route_lengths.double() - base).float()
    whole, = torch.autograd.grad(out.log_probs, leaf, grad_outputs=adv / N, retain_graph=True)
    parts = []
    for k in range(N // chunk):
        w = torch.zeros_like(adv)
        w[..., k * chunk:(k + 1) * chunk] = adv[..., k * chunk:(k + 1) * chunk] / chunk
        parts.append(torch.autograd.grad(out.log_probs, leaf, grad_outputs=w, retain_graph=True)[0].double())
    parts = torch.stack(parts).cpu().numpy()                     # [32, B, H, W]
    est, se = whole.double().cpu().numpy(), parts.std(0, ddof=1) / np.sqrt(parts.shape[0])
    assert np.abs(parts.mean(0) - est).max() <= 1e-5 * max(1.0, np.abs(est).max())   # (the chunks' mean is the one call for all samples)
    for b in range(B):
        fd = np.zeros((H, W))
        for n in np.flatnonzero((passable[b].reshape(-1) != 0) & (goal[b].reshape(-1) == 0)):
            hi, lo = cost[b].copy(), cost[b].copy()
            hi.reshape(-1)[n] = f32(cost[b].reshape(-1)[n] + f32(1e-3))      # fp32-representable steps: soft_field reads fp32 costs
            lo.reshape(-1)[n] = f32(cost[b].reshape(-1)[n] - f32(1e-3))
            fd.reshape(-1)[n] = (expected_len(hi, b) - expected_len(lo, b)) / (f64(hi.reshape(-1)[n]) - f64(lo.reshape(-1)[n]))
        cells = (passable[b] != 0) & (goal[b] == 0)
        err, bound = np.abs(est[b] - fd), 5 * se[b] + 1e-3 * np.abs(fd).max()
        sigmas = float((err[cells] / np.where(se[b] > 0, se[b], np.inf)[cells]).max())
        print(f"map {b}: max|FD| {np.abs(fd).max():.3g}, worst |estimate - FD| {err[cells].max():.3g}, the worst cell at {sigmas:.2f} standard errors")
        assert (err[cells] <= bound[cells]).all(), (b, err[cells].max())


# ---- 4: a pure function of the inputs --------------------------------------------------------------------------------------------------------------
def _setup(H=9, W=11, B=3, S=3, N=70, K=None, tau=0.5, seed=21, sample_seed=5, shape=None):
    """maps, starts (all on passable non-goal cells with a finite field), a tape and the walkers' outputs of one call"""
    from neural_astar import ops
    cost, passable, goal = SO.random_maps(seed, B, H, W)
    K = SO.default_horizon(H, W) if K is None else K
    starts = np.zeros((B, S), np.int32)
    for b in range(B):
        far = SO.hops(goal[b], passable[b]).reshape(-1)
        starts[b] = np.flatnonzero((far > 0) & (far <= K))[-S:]
    c, g, p = _t(cost), _t(goal), _t(passable)
    tape = _forward(c, g, p, tau, K, MOORE8)
    routes, lengths, _, _, _, status = ops.soft_routes_from_tape(c, g, p, tape, _t(starts, np.int32), tau, K, N, sample_seed, shape=shape)
    assert (status == 0).all()
    up = _t(np.random.default_rng(sample_seed).standard_normal((B, S, N)))
    return dict(c=c, g=g, p=p, tape=tape, starts=_t(starts, np.int32), routes=routes, lengths=lengths, status=status, up=up, tau=tau, K=K)


def _back(s, **over):
    from neural_astar import ops
    a = dict(s, **over)
    grad, st = ops.soft_routes_backward(a["c"], a["g"], a["p"], a["tape"], a["starts"], a["routes"], a["lengths"], a["status"], a["up"], a["tau"],
                                        a["K"], MOORE8)
    return grad.cpu().numpy(), st.cpu().numpy()


def test_two_calls_either_walker_shape_and_the_rest_of_the_batch():
    s = _setup()
    ref, st = _back(s)
    assert st.tolist() == [0, 0, 0] and np.count_nonzero(ref) and np.isfinite(ref).all()
    assert _same(_back(s)[0], ref) == 0                                                  # two calls
    for shape in ("lds", "gather"):                                                      # either kernel shape of the walkers
        other = _setup(shape=shape)
        assert torch.equal(other["routes"], s["routes"]) and _same(_back(other)[0], ref) == 0
    # a map alone: its rows, its plane of the tape
    B = ref.shape[0]
    for b in range(B):
        one = {k: s[k][b:b + 1].contiguous() for k in ("c", "g", "p", "starts", "routes", "lengths", "status", "up")}
        one["tape"] = s["tape"].view(B, -1)[b].contiguous()
        assert _same(_back(s, **one)[0][0], ref[b]) == 0, b


def test_two_queries_on_one_start_are_one_query_with_both_sample_sets():
    s = _setup(B=2, S=2, N=33)
    twice = s["starts"][:, :1].repeat(1, 2).contiguous()                                  # both queries on the first start
    from neural_astar import ops
    routes, lengths, _, _, _, status = ops.soft_routes_from_tape(s["c"], s["g"], s["p"], s["tape"], twice, s["tau"], s["K"], 33, 8)
    two, _ = _back(s, starts=twice, routes=routes, lengths=lengths, status=status)
    B, K = 2, s["K"]
    one, _ = _back(s, starts=twice[:, :1].contiguous(), routes=routes.reshape(B, 1, 66, K + 1), lengths=lengths.reshape(B, 1, 66),
                   status=status[:, :1].contiguous(), up=s["up"].reshape(B, 1, 66))
    assert np.count_nonzero(two) and _same(two, one) == 0


def test_doubling_every_weight_doubles_the_gradient_exactly():
    s = _setup()
    for c in (1.0, 0.37, 3.0e-12):
        g1, _ = _back(s, up=torch.full_like(s["up"], c))
        g2, _ = _back(s, up=torch.full_like(s["up"], 2 * c))
        assert np.count_nonzero(g1) and _same(g2, f32(2) * g1) == 0, c
    mixed, _ = _back(s)
    assert _same(_back(s, up=2 * s["up"])[0], f32(2) * mixed) == 0


# ---- 5: what is not read -------------------------------------------------------------------------------------------------------------------------------
def _failing_batch(bad_cost=True):
    """three 7x9 maps: failed queries of every kind beside good ones; map 1 is a BAD_COST map when asked"""
    from neural_astar import ops
    H, W, K, tau, N = 7, 9, 32, 0.5, 6
    cost, passable, goal = SO.random_maps(31, 3, H, W)
    if bad_cost:
        cost[1, 2, 3], passable[1, 2, 3] = -0.25, 1
    wall = np.flatnonzero(passable[2].reshape(-1) == 0)
    on_goal = [int(np.flatnonzero(goal[b].reshape(-1))[0]) for b in range(3)]
    free = [np.flatnonzero((SO.hops(goal[b], passable[b]).reshape(-1) > 0)) for b in range(3)]
    starts = np.array([[free[0][0], on_goal[0], -1, free[0][-1]],
                       [free[1][0], on_goal[1], H * W, free[1][-1]],
                       [int(wall[0]), on_goal[2], 2 ** 31 - 1, free[2][-1]]], np.int32)
    c, g, p = _t(cost), _t(goal), _t(passable)
    tape = _forward(c, g, p, tau, K, MOORE8)
    routes, lengths, _, _, _, status = ops.soft_routes_from_tape(c, g, p, tape, _t(starts, np.int32), tau, K, N, 3)
    up = _t(np.random.default_rng(9).standard_normal((3, 4, N)))
    return dict(c=c, g=g, p=p, tape=tape, starts=_t(starts, np.int32), routes=routes, lengths=lengths, status=status, up=up, tau=tau, K=K)


def test_the_weights_of_failed_queries_are_not_read():
    s = _failing_batch()
    status = s["status"].cpu().numpy()
    assert status.tolist() == [[0, 0, 1, 0], [9, 9, 1, 9], [3, 0, 1, 0]]
    ref, st = _back(s)
    assert st.tolist() == [0, 9, 0] and np.isfinite(ref).all() and np.count_nonzero(ref[0]) and np.count_nonzero(ref[2])
    assert _same(ref[1], np.zeros_like(ref[1])) == 0                                      # the BAD_COST map: all 0.0f
    failed = (s["status"] != 0).unsqueeze(-1).expand_as(s["up"])
    for poison in (float("nan"), float("inf"), -float("inf"), 1e30):
        got, st2 = _back(s, up=torch.where(failed, torch.full_like(s["up"], poison), s["up"]))
        assert _same(got, ref) == 0 and st2.tolist() == [0, 9, 0], poison
    # the other maps are what they are beside a good map 1 (the same walkers: a sample's number does not depend on the costs)
    good = _failing_batch(bad_cost=False)
    assert torch.equal(good["routes"][0], s["routes"][0]) and torch.equal(good["routes"][2], s["routes"][2])
    other, st3 = _back(good)
    assert st3.tolist() == [0, 0, 0] and np.count_nonzero(other[1]) and _same(other[0], ref[0]) == 0 and _same(other[2], ref[2]) == 0
    # an ok walker's NaN: its map is all NaN, the others are untouched
    for poison in (float("nan"), float("inf")):
        up = s["up"].clone()
        up[2, 1, 4] = poison
        got, st4 = _back(s, up=up)
        assert np.isnan(got[2]).all() and _same(got[:2], ref[:2]) == 0 and st4.tolist() == [0, 9, 0]


def test_goal_starts_failed_maps_and_a_map_of_one_cell_give_zeros():
    from neural_astar import ops
    s = _failing_batch()
    zeros = np.zeros((7, 9), f32)
    # a goal start contributes exactly nothing: with every other weight zero the gradient is 0.0f, whatever the goal starts' weights
    up = torch.zeros_like(s["up"])
    up[:, 1] = s["up"][:, 1]
    got, _ = _back(s, up=up)
    assert all(_same(got[b], zeros) == 0 for b in range(3))
    base, _ = _back(s, up=torch.where(torch.arange(4, device=_dev()).view(1, 4, 1) == 1, torch.zeros_like(s["up"]), s["up"]))
    small = s["up"].clone()
    small[:, 1] = 2.0 ** -8 * s["up"][:, 1].sign()        # (below every map's M_b: the scale stays what it is)
    assert _same(_back(s, up=small)[0], base) == 0 and np.count_nonzero(base)
    # an all-failed map: every start outside the map or on an obstacle
    starts = s["starts"].clone()
    starts[2] = torch.tensor([int(s["starts"][2, 0]), -1, 63, -5], dtype=torch.int32)
    routes, lengths, _, _, _, status = ops.soft_routes_from_tape(s["c"], s["g"], s["p"], s["tape"], starts, s["tau"], s["K"], 6, 3)
    assert (status[2] != 0).all()
    got, st = _back(s, starts=starts, routes=routes, lengths=lengths, status=status, up=torch.full_like(s["up"], float("nan")).where(status.unsqueeze(-1) != 0, s["up"]))
    assert _same(got[2], zeros) == 0 and _same(got[1], zeros) == 0 and st.tolist() == [0, 9, 0] and np.isfinite(got).all()
    # all weights zero: M_b = 0
    got, _ = _back(s, up=torch.zeros_like(s["up"]))
    assert _same(got, np.zeros_like(got)) == 0
    # a map of one cell
    one = _t(np.ones((1, 1, 1)))
    leaf = one.clone().requires_grad_(True)
    out = ops.soft_routes(leaf, one, one, torch.zeros(1, 2, dtype=torch.int32, device=_dev()), 0.5, 4, 5, 1, differentiable=True)
    out.log_probs.backward(torch.ones_like(out.log_probs))
    assert (out.status == 0).all() and _same(leaf.grad.cpu().numpy(), np.zeros((1, 1, 1), f32)) == 0


# ---- 6: the limit --------------------------------------------------------------------------------------------------------------------------------------
def test_the_largest_map_and_what_is_refused_before_a_launch():
    from neural_astar import ops
    H, W, K, tau, S, N = 64, 96, 16, 0.5, 4, 75
    assert H * W == ops.SOFT_ROUTES_GRAD_MAX_CELLS
    cost, passable, goal = SO.random_maps(17, 1, H, W)
    rng = np.random.default_rng(18)
    goal[0].reshape(-1)[rng.choice(np.flatnonzero(passable[0].reshape(-1) != 0), 3, replace=False)] = 1     # four goals
    far = SO.hops(goal[0], passable[0]).reshape(-1)
    near = np.flatnonzero((far > 0) & (far <= K))
    starts = near[np.argsort(far[near], kind="stable")[-S:]][None].astype(np.int32)                         # within 16 moves of a goal
    c, g, p = _t(cost), _t(goal), _t(passable)
    leaf = c.clone().requires_grad_(True)
    out = ops.soft_routes(leaf, g, p, _t(starts, np.int32), tau, K, N, 77, differentiable=True)
    assert (out.status == 0).all()
    up = np.random.default_rng(19).standard_normal((1, S, N)).astype(f32)
    out.log_probs.backward(_t(up))
    want = _expected(c, g, p, _forward(c, g, p, tau, K, MOORE8), out.routes.cpu().numpy(), out.route_lengths.cpu().numpy(), starts,
                     out.status.cpu().numpy(), up, K, tau, MOORE8)
    got = leaf.grad.cpu().numpy()
    assert np.count_nonzero(got) and _same(got, want) == 0
    # refused before anything is launched
    big = torch.ones(1, 1, 1, 6145, device=_dev(), requires_grad=True)
    with pytest.raises(NotImplementedError, match="6144.*12288"):
        ops.soft_routes(big, big, big, torch.zeros(1, 1, dtype=torch.int32, device=_dev()), tau, seed=1, differentiable=True)
    with pytest.raises(ValueError, match="max_route_len"):
        ops.soft_routes(leaf, g, p, _t(starts, np.int32), tau, K, N, 77, max_route_len=K, differentiable=True)
    with pytest.raises(NotImplementedError, match="differentiable"):
        ops.soft_routes_tiled(leaf, g, p, _t(starts, np.int32), tau, K, N, 77, differentiable=True)
    ops.soft_routes(leaf, g, p, _t(starts, np.int32), tau, K, N, 77, max_route_len=K + 1, differentiable=True)   # (exactly horizon + 1 is taken)


# ---- 7: the surface ------------------------------------------------------------------------------------------------------------------------------------
def test_only_log_probs_requires_grad_and_saved_tensors_are_checked():
    from neural_astar import ops
    cost, passable, goal = SO.random_maps(5, 2, 8, 8)
    leaf = _t(cost).requires_grad_(True)
    g, p = _t(goal), _t(passable)
    st = _t(RO.case_starts(3, 3, passable, goal), np.int32)
    plain = ops.soft_routes(leaf, g, p, st, 0.5, None, 4, 9, visits=True)
    assert not any(x.requires_grad for x in plain)                                        # the default call: as it was
    out = ops.soft_routes(leaf, g, p, st, 0.5, None, 4, 9, visits=True, differentiable=True)
    assert [name for name, x in zip(out._fields, out) if x.requires_grad] == ["log_probs"]
    for x, y in zip(out, plain):
        assert torch.equal(x.detach(), y)                                                 # the same samples, the same bits
    with torch.no_grad():
        assert not ops.soft_routes(leaf, g, p, st, 0.5, None, 4, 9, differentiable=True).log_probs.requires_grad
    assert not ops.soft_routes(leaf.detach(), g, p, st, 0.5, None, 4, 9, differentiable=True).log_probs.requires_grad
    loss = ops.route_score_loss(out.log_probs, out.route_lengths, out.status)
    loss.backward()
    assert torch.isfinite(leaf.grad).all() and leaf.grad.abs().sum() > 0
    lp = ops.soft_routes(leaf, g, p, st, 0.5, None, 4, 9, differentiable=True).log_probs
    first, = torch.autograd.grad(torch.where(torch.isfinite(lp), lp, torch.zeros_like(lp)).sum(), leaf, create_graph=True)
    assert torch.isfinite(first).all() and not first.requires_grad                        # once-differentiable: no gradient of the gradient
    again = ops.soft_routes(leaf, g, p, st, 0.5, None, 4, 9, differentiable=True)
    again.routes[0, 0, 0, 0] = 0                                                          # an in-place write to what the backward reads
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        again.log_probs.sum().backward()


def test_route_score_loss_trains_the_encoder():
    """(The planners' differentiable call is ``sample_routes_differentiable``, a method of its own: tests/test_soft_routes.py pins the
    signature of ``sample_routes``, so it takes no new keyword.)"""
    from neural_astar import ops, planner
    from neural_astar.utils import synthetic as syn
    P = syn.random_obstacle_maps(8, 32, 32, 0.25, seed=3)
    maps, goals = _t(P.map_designs), _t(P.goal_maps)
    starts = _t(RO.case_starts(1, 3, P.map_designs[:, 0], P.goal_maps[:, 0]), np.int32)
    torch.manual_seed(0)
    na = planner.NeuralAstar(encoder_input="m", encoder_arch="CNN", encoder_depth=4).to(_dev()).train()
    out = na.sample_routes_differentiable(maps, starts, goals, 0.3, num_samples=16, seed=9)
    assert out.log_probs.requires_grad and not out.routes.requires_grad and (out.status == 0).any()
    ops.route_score_loss(out.log_probs, out.route_lengths, out.status).backward()
    grads = [q.grad for q in na.encoder.parameters() if q.requires_grad]
    assert grads and all(x is not None and torch.isfinite(x).all() for x in grads) and any(x.abs().sum() > 0 for x in grads)
    # ``sample_routes`` itself is the evaluation call it was
    assert not na.sample_routes(maps, starts, goals, 0.3, num_samples=16, seed=9).log_probs.requires_grad


def test_a_captured_backward_replays_the_eager_bits():
    from neural_astar import ops
    s = _setup(H=16, W=16, B=2, S=3, N=70, K=64)
    args = (s["c"], s["g"], s["p"], s["tape"], s["starts"], s["routes"], s["lengths"], s["status"], s["up"], s["tau"], s["K"], MOORE8)
    eager = ops.soft_routes_backward(*args)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.soft_routes_backward(*args)                                                   # (warm-up on the capture stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = ops.soft_routes_backward(*args)
    for _ in range(2):                                                                    # (the second replay: the zeroing of the planes is part of the graph)
        graph.replay()
        torch.cuda.synchronize()
        for x, y in zip(captured, eager):
            assert torch.equal(x, y)
