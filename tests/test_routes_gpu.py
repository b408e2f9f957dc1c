"""GPU (-m gpu): ``plan_routes()`` / ``ops.search_routes`` on every kernel family the forward has, against the numpy route oracle
(tests/route_oracle.py, pinned on the CPU by tests/test_routes.py).

Every case checks the same things (``_check``): ``histories`` and ``paths`` equal ``forward()``'s, bitwise; ``routes`` and
``route_lengths`` equal the oracle's exactly, the -1 tail included; ``route_costs`` is within 1 float32 ulp of float32(float64 sum) --
float64 accumulation error is far below half a float32 ulp, so only a rounding tie can differ.
"""
import functools

import numpy as np
import pytest
import torch

import golden_util as G
import heuristic_oracle as HO
import neighbor_golden as NG
import route_oracle as RO

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _coupling_possible(g_ratio):
    return not (0.5 <= float(g_ratio) < 1.0)


def _module(g_ratio=0.5, Tmax=1.0, training=False, mask=HO.MOORE8, check_solvable=True, unit_cost="auto"):
    from neural_astar.planner.differentiable_astar import DifferentiableAstar
    m = DifferentiableAstar(g_ratio=g_ratio, Tmax=Tmax, check_solvable=check_solvable, unit_cost=unit_cost).to(_dev())
    if mask != HO.MOORE8:
        with torch.no_grad():
            m.neighbor_filter.copy_(torch.tensor([float((mask >> i) & 1) for i in range(9)], device=_dev()).reshape(1, 1, 3, 3))
    m.train(training)
    return m


@functools.lru_cache(maxsize=None)
def _case(kind, name):
    """(inputs as numpy, mask, h0, g_ratio, Tmax, training, the oracle's routes) of one golden -- computed once, shared, never modified"""
    if kind == "search":
        g = G.load(name)
        c, s, go, p, mask, h0 = g.cost_maps, g.start_maps, g.goal_maps, g.passable, HO.MOORE8, None
    elif kind == "neighbors":
        g = NG.load(name)
        c, s, go, p, mask, h0 = g.cost_maps, g.start_maps, g.goal_maps, g.map_designs, NG.mask_of(g.filter), None
    else:
        g = HO.load(name)
        c, s, go, p, mask, h0 = g.cost_maps, g.start_maps, g.goal_maps, g.map_designs, g.mask, g.h0
    B = c.shape[0]
    lock = B > 1 and (_coupling_possible(g.g_ratio) or h0 is not None)  # the module's own rule for the exact batch loop
    r = RO.plan(c, s, go, p, g.g_ratio, g.max_iters, mask, h0=h0, lockstep=lock)
    assert np.array_equal(r.paths, g.paths[:, 0]) and np.array_equal(r.histories, g.histories[:, 0])  # (the oracle stands on the reference)
    same = c is p or np.array_equal(c, p)
    return c, s, go, p, same, mask, h0, g.g_ratio, g.Tmax, g.training, g.max_iters, r


def _check(out, fwd, r, cap, what):
    assert not out.histories.requires_grad and not out.paths.requires_grad and not out.route_costs.requires_grad
    assert out.histories.dtype == torch.float32 and out.paths.dtype == torch.int64
    assert out.routes.dtype == torch.int32 and out.route_lengths.dtype == torch.int32 and out.route_costs.dtype == torch.float32
    B = len(r.routes)
    assert tuple(out.routes.shape) == (B, cap) and tuple(out.route_lengths.shape) == (B,) and tuple(out.route_costs.shape) == (B,)
    if fwd is not None:
        assert torch.equal(out.histories, fwd.histories.detach()), f"{what}: histories differ from forward()"
        assert torch.equal(out.paths, fwd.paths), f"{what}: paths differ from forward()"
    if r.histories is not None:
        assert np.array_equal(out.histories[:, 0].cpu().numpy(), r.histories) and np.array_equal(out.paths[:, 0].cpu().numpy(), r.paths), what
    routes, lengths, costs = out.routes.cpu().numpy(), out.route_lengths.cpu().numpy(), out.route_costs.cpu().numpy()
    assert np.array_equal(lengths, r.lengths), f"{what}: lengths {lengths.tolist()} != oracle {r.lengths.tolist()}"
    assert np.array_equal(lengths, out.paths.reshape(B, -1).sum(1).cpu().numpy())
    want = RO.rows(r, cap)
    bad = np.flatnonzero((routes != want).any(1))
    assert bad.size == 0, f"{what}: routes differ from the oracle on maps {bad.tolist()[:8]} (tail of -1 included)"
    ref32 = r.costs.astype(np.float32)
    err = np.abs(costs.astype(np.float64) - ref32.astype(np.float64))
    print(f"{what}: cap {cap}, lengths {int(lengths.min())}..{int(lengths.max())}, max cost error {err.max():.3e} (1 ulp >= {np.abs(np.spacing(ref32)).min():.3e})")
    assert (err <= np.abs(np.spacing(ref32))).all(), f"{what}: route_costs beyond 1 float32 ulp of float32(float64 sum): {err.max():.3e}"


def _run_golden(kind, name, unit_cost="auto", max_route_len=None, check_solvable=True):
    c, s, go, p, same, mask, h0, g_ratio, Tmax, training, max_iters, r = _case(kind, name)
    m = _module(g_ratio, Tmax, training, mask, check_solvable, unit_cost)
    ct, st, gt = _t(c), _t(s), _t(go)
    pt = ct if same else _t(p)
    ht = _t(h0) if h0 is not None else None
    with torch.no_grad():
        fwd = m(ct, st, gt, pt, heuristic_maps=ht)
    out = m.plan_routes(ct, st, gt, pt, heuristic_maps=ht, max_route_len=max_route_len)
    H, W = c.shape[-2:]
    cap = max_route_len if max_route_len is not None else min(H * W, max_iters + 1)
    _check(out, fwd, r, cap, f"{kind}/{name}")
    return m, out, r


# ---- the kernel families ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["grad_rand16_eval_g080", "rand32_ucost_g050", "maze32_cnncost_g050", "rand64_ucost_g050"])
def test_hand_scheduled_streams(name):
    _run_golden("search", name)


@pytest.mark.parametrize("name", ["maze32_vanilla_g050", "rand64_vanilla_g050"])
def test_unit_cost_layout(name):
    """VanillaAstar(unit_cost=True): cost map and obstacle map are ONE tensor, the LDS state has no cost word"""
    from neural_astar.planner import VanillaAstar
    c, s, go, p, same, mask, h0, g_ratio, Tmax, training, max_iters, r = _case("search", name)
    assert same
    va = VanillaAstar(g_ratio=g_ratio).to(_dev()).eval()
    va.astar.unit_cost = True
    fwd = va(_t(c), _t(s), _t(go))
    out = va.plan_routes(_t(c), _t(s), _t(go))
    _check(out, fwd, r, min(c.shape[-2] * c.shape[-1], max_iters + 1), f"unit/{name}")
    _run_golden("search", name, unit_cost=True)  # (DifferentiableAstar itself, one tensor as cost and obstacle map)


@pytest.mark.parametrize("name", ["grad_rand7x5_eval_g050", "rand20x45_ucost_g050"])
def test_compiled_loops(name):
    _run_golden("search", name)


@pytest.mark.parametrize("name", ["rand32_vn_ucost_g050", "rand16_upleft_ucost_g050"])
def test_masked(name):
    _run_golden("neighbors", name)


@pytest.mark.parametrize("name", ["zero32_ucost_g050", "field20x45_ucost_g020"])
def test_heuristic(name):
    _run_golden("heuristics", name)


@pytest.mark.parametrize("kind,name", [("neighbors", "rand80_asym_ucost_g050"), ("search", "rand100_vanilla_g050")])
def test_large_map_kernel(kind, name):
    from neural_astar import ops
    c = _case(kind, name)[0]
    assert not ops.in_lds(c.shape[-2], c.shape[-1])  # 80x80 is the smallest size the large-map kernel takes
    _run_golden(kind, name)


@pytest.mark.parametrize("name", ["maze32_train_T005", "maze32_train_T025"])
def test_budget_truncated_training_mode(name):
    m, out, r = _run_golden("search", name)
    assert m.training and not r.reached.all()  # some budget ran out: those routes need not begin at the start


# ---- the exact batch loop --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["coupled_forward_g020", "coupled_signed_g050"])
def test_exact_batch_loop(name):
    """The inputs of coupled_forward_g020 (loaded as tests/test_coupled_forward.py does) against the LOCK-STEP oracle: g_ratio 0.2 runs the
    exact pipeline straight away, and its FINAL launch rewrites the routes of the maps it re-runs.  So that the test cannot pass vacuously, at
    least one map must differ from itself searched alone.  On coupled_forward_g020 the reference's own batch run and its searched-alone run
    mark the SAME paths (tests/test_coupled_forward.py asserts it: 'same paths either way'), so the routes of that file cannot differ --
    oracle: lengths [18, 23, 13] both ways; what differs there is histories (2 cells), which plan_routes must match bitwise.  The assertion
    on the ROUTES is made on coupled_signed_g050 (negative costs at g_ratio 0.5: the launch reports NASTAR_SUMMARY_COUPLED and is repeated
    exactly), where the routes of maps 0, 1 and 2 differ from their searched-alone routes."""
    assert name not in G.names()
    g = G.load(name)
    c, s, go, p, g_ratio, max_iters = g.cost_maps, g.start_maps, g.goal_maps, g.passable, g.g_ratio, g.max_iters
    assert g.B > 1 and (_coupling_possible(g_ratio) or float(c.min()) < 0)
    lock = RO.plan(c, s, go, p, g_ratio, max_iters, lockstep=True)
    assert np.array_equal(lock.paths, g.paths[:, 0]) and np.array_equal(lock.histories, g.histories[:, 0])  # the reference's batch run
    alone = RO.plan(c, s, go, p, g_ratio, max_iters, lockstep=False)
    differs = [b for b in range(c.shape[0]) if alone.routes[b] != lock.routes[b]]
    if name == "coupled_signed_g050":
        assert differs, "no map's route differs from its searched-alone route: the test would pass without the exact batch loop"
    else:
        assert not np.array_equal(alone.histories, lock.histories)
    m = _module(g_ratio)
    ct, st, gt, pt = _t(c), _t(s), _t(go), _t(p)
    with torch.no_grad():
        fwd = m(ct, st, gt, pt)
    out = m.plan_routes(ct, st, gt, pt)
    H, W = c.shape[-2:]
    _check(out, fwd, lock, min(H * W, max_iters + 1), f"exact/{name}")


def test_exact_batch_loop_on_the_large_map_kernel():
    """80x80 maps at g_ratio 0.2: marks + lock-step re-run on the kernel whose parents live in the HBM slab"""
    c, s, go, p, same, mask, h0, _, _, _, max_iters, _ = _case("neighbors", "rand80_asym_ucost_g050")
    lock = RO.plan(c, s, go, p, 0.2, max_iters, mask, lockstep=True)
    m = _module(0.2, mask=mask)
    ct, st, gt, pt = _t(c), _t(s), _t(go), _t(p)
    with torch.no_grad():
        fwd = m(ct, st, gt, pt)
    out = m.plan_routes(ct, st, gt, pt)
    _check(out, fwd, lock, min(80 * 80, max_iters + 1), "exact/large")


# ---- degenerate maps -------------------------------------------------------------------------------------------------------------------------
def _degenerate(H, W):
    """map 0: start == goal; map 1: the goal walled in; map 2: no goal at all; map 3: an ordinary map"""
    B = 4
    c = np.ones((B, 1, H, W), np.float32)
    s = np.zeros_like(c)
    g = np.zeros_like(c)
    s[:, 0, 1, 1] = 1
    g[0, 0, 1, 1] = 1
    g[1, 0, H - 2, W - 2] = 1
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            if dr or dc:
                c[1, 0, H - 2 + dr, W - 2 + dc] = 0
    g[3, 0, H - 1, W - 1] = 1
    return c, s, g


@pytest.mark.parametrize("H,W,unit", [(32, 32, False), (32, 32, True), (7, 5, False), (80, 80, False)])
def test_degenerate_maps(H, W, unit):
    c, s, g = _degenerate(H, W)
    m = _module(check_solvable=False, unit_cost=True if unit else "auto")
    ct = _t(c)
    with torch.no_grad():
        fwd = m(ct, _t(s), _t(g), ct)
    out = m.plan_routes(ct, _t(s), _t(g), ct, max_route_len=H * W)
    r = RO.plan(c, s, g, c, 0.5, W * W)  # the module's budget: int(Tmax * W * W) steps (7x5: 25, fewer than the 26 cells map 1 can close)
    goal1 = (H - 2) * W + (W - 2)
    assert r.routes[0] == [W + 1] and r.routes[1] == [goal1] and r.routes[2] == [] and r.routes[3][0] == W + 1 and r.routes[3][-1] == H * W - 1
    _check(out, fwd, r, H * W, f"degenerate {H}x{W} unit={unit}")
    assert out.route_lengths.tolist()[:3] == [1, 1, 0] and out.route_costs.tolist()[:3] == [0.0, 0.0, 0.0]
    assert out.routes[0, 0].item() == W + 1 and out.routes[1, 0].item() == goal1 and (out.routes[2] == -1).all()
    with pytest.raises(Exception, match="no start->goal route"):  # any other check_solvable value reads the status before returning
        _module().plan_routes(ct, _t(s), _t(g), ct)


def test_refused_maps_have_empty_routes():
    """per-map status NASTAR_ERR_NOT_UNIT_COST / NASTAR_ERR_BAD_HEURISTIC: the route is empty, length 0; the other maps are searched"""
    c, s, go, p, same, mask, h0, g_ratio, Tmax, training, max_iters, r = _case("search", "maze32_vanilla_g050")
    c = c[:4].copy()
    c[1, 0, 0, 0] = 0.5  # not a unit-cost map
    m = _module(check_solvable=False, unit_cost=True)
    ct = _t(c)
    out = m.plan_routes(ct, _t(s[:4]), _t(go[:4]), ct)
    assert m.last_status.tolist() == [0, 7, 0, 0]
    assert out.route_lengths.tolist() == [int(r.lengths[0]), 0, int(r.lengths[2]), int(r.lengths[3])]
    assert (out.routes[1] == -1).all() and out.route_costs[1].item() == 0.0 and out.paths[1].sum().item() == 0
    assert np.array_equal(out.routes.cpu().numpy()[[0, 2, 3]], RO.rows(r, out.routes.shape[1])[[0, 2, 3]])
    h = np.zeros((4, 1, 32, 32), np.float32)
    h[2, 0, 5, 5] = np.nan
    m = _module(check_solvable=False)
    ct = _t(_case("search", "maze32_vanilla_g050")[0][:4])
    out = m.plan_routes(ct, _t(s[:4]), _t(go[:4]), ct, heuristic_maps=_t(h))
    assert m.last_status.tolist() == [0, 0, 8, 0]
    assert out.route_lengths[2].item() == 0 and (out.routes[2] == -1).all() and out.route_costs[2].item() == 0.0
    assert (out.route_lengths[[0, 1, 3]] > 0).all() and torch.equal(out.route_lengths.long(), out.paths.reshape(4, -1).sum(1))


# ---- short rows, placement, the default path --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [8, 1])
def test_short_rows_keep_the_last_cells(cap):
    m, out, r = _run_golden("search", "maze32_vanilla_g050", max_route_len=cap)
    assert (r.lengths > 8).any()  # the true length is reported although the row is shorter
    goals = np.array([cells[-1] for cells in r.routes])
    idx = np.minimum(r.lengths, cap) - 1
    assert np.array_equal(out.routes.cpu().numpy()[np.arange(len(goals)), idx], goals)  # the goal sits at index min(len, cap) - 1
    if cap == 8:
        long = np.flatnonzero(r.lengths >= 8)
        assert np.array_equal(out.routes.cpu().numpy()[long, 7], goals[long])


def test_rows_are_indexed_by_map_whatever_the_placement():
    from neural_astar import ops
    c, s, go, p, same, mask, h0, g_ratio, Tmax, training, max_iters, r = _case("search", "rand32_ucost_g050")
    B = 16
    ct, st, gt, pt = _t(c[:B]), _t(s[:B]), _t(go[:B]), _t(p[:B])
    plain = ops.search_routes(ct, st, gt, pt, g_ratio, max_iters)
    order = torch.arange(B - 1, -1, -1, dtype=torch.int32, device=_dev())
    order_out = ops.new_placement_buffer(B, _dev())
    placed = ops.search_routes(ct, st, gt, pt, g_ratio, max_iters, order=order, order_out=order_out)
    for a, b in zip(plain, placed):
        assert torch.equal(a, b)
    assert sorted(order_out[:B].tolist()) == list(range(B))
    assert np.array_equal(placed[5].cpu().numpy(), RO.rows(r, 1024)[:B]) and np.array_equal(placed[6].cpu().numpy(), r.lengths[:B])
    cost64 = r.costs[:B].astype(np.float32)
    assert (np.abs(placed[7].cpu().numpy().astype(np.float64) - cost64) <= np.abs(np.spacing(cost64))).all()


def test_forward_is_unchanged_by_a_plan_routes_call():
    c, s, go, p, same, mask, h0, g_ratio, Tmax, training, max_iters, r = _case("search", "rand32_ucost_g050")
    m = _module(g_ratio)
    ct, st, gt, pt = _t(c), _t(s), _t(go), _t(p)
    with torch.no_grad():
        before = m(ct, st, gt, pt)
    m.plan_routes(ct, st, gt, pt, max_route_len=4)
    with torch.no_grad():
        after = m(ct, st, gt, pt)
    assert torch.equal(before.histories, after.histories) and torch.equal(before.paths, after.paths)
    cg = ct.clone().requires_grad_(True)  # ... and under autograd (plan_routes itself keeps no graph)
    routed = m.plan_routes(cg, st, gt, pt)
    assert not routed.histories.requires_grad and torch.equal(routed.histories, before.histories)
    out = m(cg, st, gt, pt)
    assert out.histories.requires_grad and torch.equal(out.histories.detach(), before.histories)


def test_neural_astar_plans_the_routes_of_its_own_cost_maps():
    from neural_astar.planner import NeuralAstar
    from neural_astar.planner.differentiable_astar import route_coords
    g = G.load("maze32_vanilla_g050")
    torch.manual_seed(0)
    na = NeuralAstar(encoder_depth=4).to(_dev()).eval()
    md, st, gt = _t(g.map_designs[:4]), _t(g.start_maps[:4]), _t(g.goal_maps[:4])
    with torch.no_grad():
        fwd = na(md, st, gt)
        cost = na.encode(md, st, gt)
        out = na.plan_routes(md, st, gt)
    r = RO.plan(cost.cpu().numpy(), g.start_maps[:4], g.goal_maps[:4], g.map_designs[:4], 0.5, 1024)
    _check(out, fwd, r, 1024, "NeuralAstar")
    rc = route_coords(out.routes, 32)
    n = int(out.route_lengths[0])
    assert rc.shape == (4, 1024, 2) and (rc[0, n:] == -1).all() and (rc[0, :n, 0] * 32 + rc[0, :n, 1] == out.routes[0, :n]).all()
