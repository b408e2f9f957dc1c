"""GPU (-m gpu): the multi-source search on the kernels (``planner.multi_source = True``, include/nastar_sources.h) -- against the reference run
on multi-hot start maps (tests/golden/multisource/, tools/gen_golden_multisource.py), against the default call on one-hot inputs (identity),
and against the numpy restatement (tests/multisource_oracle.py) where the reference has no answer (a walled-in map) or no vector (tiny maps)."""
import numpy as np
import pytest
import torch

import multisource_oracle as MO

pytestmark = pytest.mark.gpu

FORWARD = [n for n in MO.names() if not n.startswith("grad_")]
GRAD = [n for n in MO.names() if n.startswith("grad_")]


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _filter_of(mask):
    return torch.tensor([float((mask >> i) & 1) for i in range(9)], dtype=torch.float32, device=_dev()).reshape(1, 1, 3, 3)


def _module(g_ratio=0.5, Tmax=1.0, training=False, mask=MO.MOORE8, check_solvable=True, multi=True):
    from neural_astar.planner.differentiable_astar import DifferentiableAstar
    m = DifferentiableAstar(g_ratio=g_ratio, Tmax=Tmax, check_solvable=check_solvable).to(_dev())
    if mask != MO.MOORE8:
        with torch.no_grad():
            m.neighbor_filter.copy_(_filter_of(mask))
    m.train(training)
    m.multi_source = multi
    return m


def _gmodule(g, check_solvable=True):
    return _module(g.g_ratio, g.Tmax, g.training, g.mask, check_solvable)


def _h0(g):
    return _t(g.h0) if g.h0 is not None else None


# ---- the reference's vectors ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("check", [True, "deferred", False])
@pytest.mark.parametrize("name", FORWARD)
def test_forward_matches_reference(name, check):
    g = MO.load(name)
    m = _gmodule(g, check)
    out = m(_t(g.cost_maps), _t(g.start_maps), _t(g.goal_maps), _t(g.map_designs), heuristic_maps=_h0(g))
    if check == "deferred":
        m.raise_if_unsolvable()
    assert np.array_equal(out.histories.cpu().numpy(), g.histories), f"{name}: histories differ from the reference"
    assert np.array_equal(out.paths.cpu().numpy(), g.paths), f"{name}: paths differ from the reference"
    assert int(m.last_iters.max()) - 1 == g.t_batch  # the reference's loop index at its break
    assert (m.last_status == 0).all()


@pytest.mark.parametrize("name", FORWARD)
def test_forward_under_autograd_matches_reference(name):
    g = MO.load(name)
    m = _gmodule(g)
    cost = _t(g.cost_maps).requires_grad_(True)
    out = m(cost, _t(g.start_maps), _t(g.goal_maps), _t(g.map_designs), heuristic_maps=_h0(g))
    assert out.histories.requires_grad
    assert np.array_equal(out.histories.detach().cpu().numpy(), g.histories) and np.array_equal(out.paths.cpu().numpy(), g.paths)


def test_the_default_call_takes_the_highest_index_start_only():
    """what ``multi_source = False`` documents: on a multi-hot start map it is the search from the LAST non-zero cell, not the reference's"""
    g = MO.load("unit32_k4")
    B, _, H, W = g.map_designs.shape
    last = np.zeros((B, H * W), np.float32)
    last[np.arange(B), [int(np.flatnonzero(g.start_maps[b].reshape(-1))[-1]) for b in range(B)]] = 1
    m = _module(multi=False, check_solvable=False)
    a = m(_t(g.cost_maps), _t(g.start_maps), _t(g.goal_maps), _t(g.map_designs))
    b = m(_t(g.cost_maps), _t(last.reshape(B, 1, H, W)), _t(g.goal_maps), _t(g.map_designs))
    assert torch.equal(a.histories, b.histories) and torch.equal(a.paths, b.paths)
    assert not np.array_equal(a.histories.cpu().numpy(), g.histories)


@pytest.mark.parametrize("name", FORWARD)
def test_selection_logs_match_reference(name):
    from neural_astar import ops
    g = MO.load(name)
    B = g.map_designs.shape[0]
    hist, paths, iters, status, log = ops.search_nograd(_t(g.cost_maps), _t(g.start_maps), _t(g.goal_maps), _t(g.map_designs), g.g_ratio, g.max_iters, True,
                                                        exact=B > 1, neighbor_mask=None if g.mask == MO.MOORE8 else g.mask, heuristic=_h0(g),
                                                        multi_source=True)
    assert (status == 0).all()
    iters, log = iters.cpu().numpy(), log.cpu().numpy()
    for b in range(B):
        n = int(iters[b])
        assert np.array_equal(log[b, :n], g.sel_log[b, :n]), f"{name}: map {b} selects differently from the reference"
        assert (g.sel_log[b, n:] == int(g.goal_maps[b].reshape(-1).argmax())).all()
    assert np.array_equal(hist.cpu().numpy(), g.histories[:, 0])


@pytest.mark.parametrize("name", FORWARD)
def test_plan_routes_begin_at_the_winning_source(name):
    import heuristic_oracle as HO
    g = MO.load(name)
    B, _, H, W = g.map_designs.shape
    m = _gmodule(g)
    r = m.plan_routes(_t(g.cost_maps), _t(g.start_maps), _t(g.goal_maps), _t(g.map_designs), heuristic_maps=_h0(g))
    assert np.array_equal(r.histories.cpu().numpy(), g.histories) and np.array_equal(r.paths.cpu().numpy(), g.paths)
    _, maps = MO.search(g.cost_maps, g.start_maps, g.goal_maps, g.map_designs, g.h0, g.g_ratio, g.max_iters, g.mask, lockstep=B > 1, with_maps=True)
    moves = set(HO.offsets(g.mask))
    routes, lengths, costs = r.routes.cpu().numpy(), r.route_lengths.cpu().numpy(), r.route_costs.cpu().numpy()
    for b in range(B):
        n = int(lengths[b])
        assert n == int(g.paths[b].sum())
        cells = routes[b, :n].tolist()
        assert (routes[b, n:] == -1).all()
        assert sorted(cells) == np.flatnonzero(g.paths[b].reshape(-1)).tolist(), f"map {b}: the route's cells are not the cells of the reference's paths"
        assert cells[-1] == maps[b].goal
        for a, c in zip(cells, cells[1:]):
            assert (c // W - a // W, c % W - a % W) in moves, f"map {b}: {a} -> {c} is not an allowed move"
        assert maps[b].parent[cells[0]] == MO.UNSET and cells[0] in maps[b].sources, f"map {b}: the route does not begin at a source with an unset parent"
        assert cells == maps[b].route(max(len(maps[b].sel) - 1, 0))
        want = 0.0  # fp64, in the order the kernel walks: from the goal's parent back to the source
        for c in cells[-2::-1]:
            want += float(g.cost_maps[b].reshape(-1)[c])
        assert costs[b] == np.float32(want)


def test_plan_routes_short_rows_and_the_wrappers():
    from neural_astar.planner import VanillaAstar
    g = MO.load("unit32_k4")
    va = VanillaAstar(g_ratio=g.g_ratio).to(_dev()).eval()
    va.multi_source = True
    full = va.plan_routes(_t(g.map_designs), _t(g.start_maps), _t(g.goal_maps))
    short = va.plan_routes(_t(g.map_designs), _t(g.start_maps), _t(g.goal_maps), max_route_len=3)
    assert np.array_equal(full.paths.cpu().numpy(), g.paths) and torch.equal(full.route_lengths, short.route_lengths)
    for b in range(g.map_designs.shape[0]):
        n = int(full.route_lengths[b])
        k = min(n, 3)
        assert torch.equal(short.routes[b, :k], full.routes[b, n - k:n]) and (short.routes[b, k:] == -1).all()
    out = va(_t(g.map_designs), _t(g.start_maps), _t(g.goal_maps))
    assert np.array_equal(out.histories.cpu().numpy(), g.histories)


def test_store_intermediate_results_follow_the_references_log():
    g = MO.load("unit16_samechunk")
    m = _gmodule(g)
    out = m(_t(g.cost_maps), _t(g.start_maps), _t(g.goal_maps), _t(g.map_designs), store_intermediate_results=True)
    ir = out.intermediate_results
    B, _, H, W = g.map_designs.shape
    assert len(ir) == g.t_batch + 2
    cur = np.zeros((B, H * W), np.float32)
    for t in range(g.t_batch + 1):  # entry t: the histories BEFORE step t and the one-hot of the cell selected AT step t
        assert np.array_equal(ir[t]["histories"].cpu().numpy().reshape(B, -1), cur), t
        assert np.array_equal(ir[t]["paths"].cpu().numpy().reshape(B, -1).argmax(1), g.sel_log[:, t]), t
        cur[np.arange(B), g.sel_log[:, t]] = 1.0
    assert np.array_equal(ir[-1]["histories"].cpu().numpy(), g.histories) and np.array_equal(ir[-1]["paths"].cpu().numpy(), g.paths)


@pytest.mark.parametrize("name", GRAD)
def test_l1_gradients_match_reference(name):
    g = MO.load(name)
    h0 = _t(g.h0).requires_grad_(True) if g.h0 is not None else None
    if g.h0_only:  # VanillaAstar on binary maps with a learned heuristic: the cost maps carry no graph, the backward must run all the same
        from neural_astar.planner import VanillaAstar
        va = VanillaAstar(g_ratio=g.g_ratio).to(_dev()).eval()
        va.multi_source = True
        out = va(_t(g.map_designs), _t(g.start_maps), _t(g.goal_maps), heuristic_maps=h0)
        cost = None
    else:
        cost = _t(g.cost_maps).requires_grad_(True)
        out = _gmodule(g)(cost, _t(g.start_maps), _t(g.goal_maps), _t(g.map_designs), heuristic_maps=h0)
    assert np.array_equal(out.histories.detach().cpu().numpy(), g.histories)
    torch.nn.L1Loss()(out.histories, _t(g.target)).backward()
    for what, got, ref in (("cost", cost, g.grad_cost), ("h0", h0, g.grad_h0)):
        if ref is None:
            continue
        scale = max(1.0, float(np.abs(ref).max()))
        err = float(np.abs(got.grad.cpu().numpy() - ref).max())
        print(f"{name}: max |dL/d{what} - reference| = {err:.3e} (scale {scale:.3e}, largest reference value {float(np.abs(ref).max()):.3e})")
        assert err <= 1e-5 * scale, f"{name}: max |dL/d{what} - reference| = {err:.3e}"
    if cost is not None and h0 is not None:
        assert torch.equal(h0.grad, cost.grad)


# ---- identity: one-hot inputs ------------------------------------------------------------------------------------------------------------
def _random_batch(B, H, W, seed, p=0.2):
    from neural_astar.utils import synthetic as syn
    pr = syn.random_obstacle_maps(B, H, W, p, seed=seed)
    cost = syn.random_costs(B, H, W, seed=seed + 1)
    return [_t(x) for x in (cost, pr.start_maps, pr.goal_maps, pr.map_designs)]


IDENTITY = [(6, 16, 16), (6, 32, 32), (3, 64, 64), (4, 20, 45), (2, 96, 96)]


@pytest.mark.parametrize("variant", ["moore8", "masked", "heuristic"])
@pytest.mark.parametrize("g_ratio", [0.5, 0.2])
@pytest.mark.parametrize("shape", IDENTITY, ids=lambda s: f"{s[0]}x{s[1]}x{s[2]}")
def test_one_hot_inputs_give_the_default_call_bit_for_bit(shape, g_ratio, variant):
    from neural_astar import ops
    B, H, W = shape
    cost, s, goal, p = _random_batch(B, H, W, seed=11 * sum(shape) + int(10 * g_ratio), p=0.15 if variant == "masked" else 0.2)
    mask = MO.VON_NEUMANN if variant == "masked" else MO.MOORE8
    h0 = None
    if variant == "heuristic":
        h0 = _t((np.random.Generator(np.random.PCG64(B + H)).random((B, 1, H, W)) * 2.0 + 0.5).astype(np.float32)) + ops.heuristic(goal)
    exact = B > 1 and (ops.coupling_possible(g_ratio) or h0 is not None)
    nm = None if mask == MO.MOORE8 else mask
    a = ops.search_nograd(cost, s, goal, p, g_ratio, W * W, True, exact=exact, neighbor_mask=nm, heuristic=h0)
    b = ops.search_nograd(cost, s, goal, p, g_ratio, W * W, True, exact=exact, neighbor_mask=nm, heuristic=h0, multi_source=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    ia, la, lb = a[2].cpu().numpy(), a[4].cpu().numpy(), b[4].cpu().numpy()
    for i in range(B):
        assert np.array_equal(la[i, :ia[i]], lb[i, :ia[i]]), f"map {i}: selection logs differ"
    # the modules: forward, plan_routes and the gradients
    up = _t(np.random.Generator(np.random.PCG64(5)).standard_normal((B, 1, H, W)).astype(np.float32))
    res = []
    for multi in (False, True):
        m = _module(g_ratio, mask=mask, check_solvable=False, multi=multi)
        c = cost.clone().requires_grad_(True)
        o = m(c, s, goal, p, heuristic_maps=h0)
        (o.histories * up).sum().backward()
        r = m.plan_routes(cost, s, goal, p, heuristic_maps=h0)
        res.append((o, c.grad, r))
    (o1, g1, r1), (o2, g2, r2) = res
    assert torch.equal(o1.histories, o2.histories) and torch.equal(o1.paths, o2.paths) and torch.equal(o1.histories[:, 0], a[0])
    assert all(torch.equal(x, y) for x, y in zip(r1, r2))
    if variant == "moore8" and H == W and W in (16, 32) and not exact:
        # the default call of 16x16 / 32x32 replays with the hand-scheduled loop (unless the log is a lock-step one): the project's bar
        scale = max(1.0, float(g1.abs().max()))
        assert float((g1 - g2).abs().max()) <= 1e-5 * scale
    else:  # both calls run the same compiled replay, and a single start adds the same single term to S and D: the same bits
        assert torch.equal(g1, g2)


def test_one_hot_identity_with_the_training_budget():
    cost, s, goal, p = _random_batch(6, 32, 32, seed=77)
    outs = []
    for multi in (False, True):
        m = _module(0.5, Tmax=0.25, training=True, multi=multi)
        outs.append(m(cost, s, goal, p))
        assert int(m.last_iters.max()) <= 256
    assert torch.equal(outs[0].histories, outs[1].histories) and torch.equal(outs[0].paths, outs[1].paths)


# ---- where the reference has no answer: against the restatement ---------------------------------------------------------------------------
def _walled_batch(H, W, seed):
    """4 maps; in map 1 both starts sit inside a closed ring of obstacles (the goal outside it), in map 2 one of the two does"""
    rng = np.random.Generator(np.random.PCG64(seed))
    B = 4
    maps = (rng.random((B, 1, H, W)) > 0.1).astype(np.float32)
    cost = rng.random((B, 1, H, W)).astype(np.float32)
    start = np.zeros((B, 1, H, W), np.float32)
    goal = np.zeros((B, 1, H, W), np.float32)
    for b in range(B):
        maps[b, 0, 1:4, 1:5] = 0
        maps[b, 0, 2, 2:4] = 1          # a 1 x 2 cell behind a wall
        maps[b, 0, H - 2, :] = 1        # a free row for the goal and the outside start
        goal[b, 0, H - 2, W - 2] = 1
        maps[b, 0, :, 6] = 1            # ... and a free column that leads to it
    start[0, 0, H - 2, 7] = start[0, 0, 0, 6] = 1
    start[1, 0, 2, 2] = start[1, 0, 2, 3] = 1           # all starts walled in
    start[2, 0, 2, 2] = start[2, 0, H - 2, 6] = 1       # one walled in, one free
    start[3, 0, 5, 6] = start[3, 0, H - 2, 0] = 1
    return cost, start, goal, maps


@pytest.mark.parametrize("shape", [(20, 24), (96, 96)], ids=["lds", "large"])
@pytest.mark.parametrize("g_ratio", [0.5, 0.2])
def test_a_walled_in_map_is_reported_and_its_neighbours_are_searched(shape, g_ratio):
    from neural_astar.planner.differentiable_astar import UnsolvableMapError
    H, W = shape
    cost, start, goal, maps = _walled_batch(H, W, seed=H + W)
    o = MO.search(cost, start, goal, maps, None, g_ratio, W * W, lockstep=True)
    assert o.status.tolist() == [0, MO.STATUS_UNSOLVABLE, 0, 0]
    m = _module(g_ratio, check_solvable=False)
    out = m(_t(cost), _t(start), _t(goal), _t(maps))
    assert m.last_status.cpu().tolist() == [0, 3, 0, 0]
    ok = [0, 2, 3]
    assert np.array_equal(out.histories[:, 0].cpu().numpy()[ok], o.histories[ok]) and np.array_equal(out.paths[:, 0].cpu().numpy()[ok], o.paths[ok])
    assert np.array_equal(out.histories[1, 0].cpu().numpy(), o.histories[1])  # the two cells behind the wall, closed
    with pytest.raises(UnsolvableMapError, match=r"\[1\]"):
        _module(g_ratio, check_solvable=True)(_t(cost), _t(start), _t(goal), _t(maps))


def test_a_map_without_a_start_cell_is_unsolvable():
    cost, start, goal, maps = _walled_batch(20, 24, seed=3)
    start[0] = 0
    m = _module(check_solvable=False)
    out = m(_t(cost), _t(start), _t(goal), _t(maps))
    assert m.last_status.cpu().tolist() == [3, 3, 0, 0] and out.histories[0].sum() == 0


@pytest.mark.parametrize("shape", [(7, 5), (1, 9), (1, 2), (1, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("g_ratio", [0.5, 0.2])
def test_tiny_maps_against_the_restatement(shape, g_ratio):
    H, W = shape
    rng = np.random.Generator(np.random.PCG64(H * 10 + W))
    B = 3
    maps = np.ones((B, 1, H, W), np.float32)
    cost = rng.random((B, 1, H, W)).astype(np.float32)
    start = np.zeros((B, H * W), np.float32)
    goal = np.zeros((B, H * W), np.float32)
    for b in range(B):
        cells = rng.permutation(H * W)
        goal[b, cells[0]] = 1
        start[b, cells[1:3] if H * W > 2 else cells[-1:]] = 1  # two starts where the map has room for them beside the goal
    if H * W == 1:
        start[:] = 1  # 1x1: the one cell is start and goal
    start, goal = start.reshape(B, 1, H, W), goal.reshape(B, 1, H, W)
    o, states = MO.search(cost, start, goal, maps, None, g_ratio, W * W, lockstep=True, with_maps=True)
    m = _module(g_ratio, check_solvable=False)
    out = m(_t(cost), _t(start), _t(goal), _t(maps))
    assert np.array_equal(m.last_status.cpu().numpy(), o.status)
    ok = o.status == 0
    assert np.array_equal(out.histories[:, 0].cpu().numpy()[ok], o.histories[ok]) and np.array_equal(out.paths[:, 0].cpu().numpy()[ok], o.paths[ok])
    r = m.plan_routes(_t(cost), _t(start), _t(goal), _t(maps))
    for b in np.flatnonzero(ok):
        n = int(r.route_lengths[b])
        assert r.routes[b, :n].cpu().tolist() == states[b].route(max(len(states[b].sel) - 1, 0))


# ---- the lanes that search from one start cell per map --------------------------------------------------------------------------------------
def test_fused_l1_step_trains_a_multi_source_planner_through_the_planner():
    """the training step of PlannerModule / utils.distributed: same loss, histories and gradient as planner(...) + L1Loss, i.e. the reference's"""
    from neural_astar.planner import VanillaAstar
    from neural_astar.utils import training
    g = MO.load("grad_unit32_train_T025_k3")
    va = VanillaAstar(g_ratio=g.g_ratio).to(_dev())
    va.astar.Tmax = g.Tmax
    va.train()
    va.multi_source = True
    maps = _t(g.map_designs).requires_grad_(True)
    loss, out = training.fused_l1_step(va, maps, _t(g.start_maps), _t(g.goal_maps), _t(g.target))
    assert np.array_equal(out.histories.detach().cpu().numpy(), g.histories)
    loss.backward()
    err = float(np.abs(maps.grad.cpu().numpy() - g.grad_cost).max())
    assert err <= 1e-5 * max(1.0, float(np.abs(g.grad_cost).max())), err


def test_in_flight_planner_refuses_and_the_validation_pair_honours_multi_source():
    from neural_astar.parallel import InFlightPlanner
    from neural_astar.planner import NeuralAstar, VanillaAstar
    from neural_astar.utils import metrics
    g = MO.load("unit32_k4")
    maps, s, goal = _t(g.map_designs), _t(g.start_maps), _t(g.goal_maps)
    va = VanillaAstar().to(_dev()).eval()
    va.multi_source = True
    with pytest.raises(NotImplementedError, match="multi_source"):
        InFlightPlanner(va).submit(maps, s, goal)
    na = NeuralAstar(encoder_depth=1).to(_dev()).eval()
    na.multi_source = True
    a, b = metrics.plan_with_vanilla(na, maps, s, goal)  # one launch through planner.astar: both halves from every start
    assert np.array_equal(b.histories.cpu().numpy(), g.histories) and np.array_equal(b.paths.cpu().numpy(), g.paths)
    na.train()  # the two-launch branch: its own VanillaAstar gets the flag
    with torch.no_grad():
        a, b = metrics.plan_with_vanilla(na, maps, s, goal)
    assert np.array_equal(b.histories.cpu().numpy(), g.histories)
