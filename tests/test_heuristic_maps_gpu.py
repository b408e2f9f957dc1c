"""GPU (-m gpu): ``forward(..., heuristic_maps=)`` on the kernels -- against the reference run with a replaced get_heuristic
(tests/golden/heuristics/, tools/gen_golden_heuristic.py), against the call without a heuristic when the tensor holds the built-in one
(identity sweep), against the numpy restatement (tests/heuristic_oracle.py) on random inputs, and a NaN in one map's heuristic."""
import numpy as np
import pytest
import torch

import heuristic_oracle as HO

pytestmark = pytest.mark.gpu

FORWARD = [n for n in HO.names() if not n.startswith("grad_")]
GRAD = [n for n in HO.names() if n.startswith("grad_")]


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _filter_of(mask):
    return torch.tensor([float((mask >> i) & 1) for i in range(9)], dtype=torch.float32, device=_dev()).reshape(1, 1, 3, 3)


def _module(g_ratio=0.5, Tmax=1.0, training=False, mask=HO.MOORE8, check_solvable=True):
    from neural_astar.planner.differentiable_astar import DifferentiableAstar
    m = DifferentiableAstar(g_ratio=g_ratio, Tmax=Tmax, check_solvable=check_solvable).to(_dev())
    if mask != HO.MOORE8:
        with torch.no_grad():
            m.neighbor_filter.copy_(_filter_of(mask))
    m.train(training)
    return m


def _gmodule(g, check_solvable=True):
    return _module(g.g_ratio, g.Tmax, g.training, g.mask, check_solvable)


# ---- the reference's vectors ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grad", [False, True])
@pytest.mark.parametrize("check", [True, "deferred", False])
@pytest.mark.parametrize("name", FORWARD)
def test_forward_matches_reference(name, check, grad):
    g = HO.load(name)
    m = _gmodule(g, check)
    cost = _t(g.cost_maps).requires_grad_(grad)
    with torch.set_grad_enabled(grad):
        out = m(cost, _t(g.start_maps), _t(g.goal_maps), _t(g.map_designs), heuristic_maps=_t(g.h0))
    if check == "deferred":
        m.raise_if_unsolvable()
    assert np.array_equal(out.histories.detach().cpu().numpy(), g.histories), f"{name}: histories differ from the reference"
    assert np.array_equal(out.paths.cpu().numpy(), g.paths), f"{name}: paths differ from the reference"
    assert int(m.last_iters.max()) - 1 == g.t_batch  # the reference's loop index at its break
    assert (m.last_status == 0).all()


@pytest.mark.parametrize("name", FORWARD)
def test_selection_logs_match_reference(name):
    g = HO.load(name)
    cost, s, goal, p, h0 = (_t(x)[:, 0] for x in (g.cost_maps, g.start_maps, g.goal_maps, g.map_designs, g.h0))
    hist, paths, iters, status, log = torch.ops.nastar.astar_forward(cost, s, goal, p, g.g_ratio, g.max_iters, True, 0, 0, cost.shape[0] > 1, g.mask, h0)
    assert (status == 0).all()
    iters, log = iters.cpu().numpy(), log.cpu().numpy()
    for b in range(cost.shape[0]):
        n = int(iters[b])
        assert np.array_equal(log[b, :n], g.sel_log[b, :n]), f"{name}: map {b} selects differently from the reference"
        assert (g.sel_log[b, n:] == int(g.goal_maps[b].reshape(-1).argmax())).all()  # ... and sits at its fixed point for the rest of the loop
    assert np.array_equal(hist.cpu().numpy(), g.histories[:, 0])


def test_store_intermediate_results_follow_the_references_log():
    g = HO.load("coupled_field24_ucost_g050")
    m = _gmodule(g)
    out = m(_t(g.cost_maps), _t(g.start_maps), _t(g.goal_maps), _t(g.map_designs), store_intermediate_results=True, heuristic_maps=_t(g.h0))
    ir = out.intermediate_results
    B, _, H, W = g.map_designs.shape
    assert len(ir) == g.t_batch + 2
    cur = np.zeros((B, H * W), np.float32)
    for t in range(g.t_batch + 1):  # entry t: the histories BEFORE step t and the one-hot of the cell selected AT step t
        if t in (0, 1, 2, g.t_batch // 2, g.t_batch - 1, g.t_batch):
            assert np.array_equal(ir[t]["histories"].cpu().numpy().reshape(B, -1), cur), t
            assert np.array_equal(ir[t]["paths"].cpu().numpy().reshape(B, -1).argmax(1), g.sel_log[:, t]), t
        cur[np.arange(B), g.sel_log[:, t]] = 1.0
    assert np.array_equal(ir[-1]["histories"].cpu().numpy(), g.histories) and np.array_equal(ir[-1]["paths"].cpu().numpy(), g.paths)


@pytest.mark.parametrize("name", GRAD)
def test_l1_gradients_match_reference(name):
    g = HO.load(name)
    h0 = _t(g.h0).requires_grad_(True)
    if g.h0_only:  # VanillaAstar on binary maps with a learned heuristic: the cost maps carry no graph, the backward must run all the same
        from neural_astar.planner import VanillaAstar
        assert g.mask == HO.MOORE8 and not g.training
        va = VanillaAstar(g_ratio=g.g_ratio).to(_dev()).eval()
        out = va(_t(g.map_designs), _t(g.start_maps), _t(g.goal_maps), heuristic_maps=h0)
        cost = None
    else:
        cost = _t(g.cost_maps).requires_grad_(True)
        out = _gmodule(g)(cost, _t(g.start_maps), _t(g.goal_maps), _t(g.map_designs), heuristic_maps=h0)
    assert np.array_equal(out.histories.detach().cpu().numpy(), g.histories)
    torch.nn.L1Loss()(out.histories, _t(g.target)).backward()
    ref = g.grad_h0
    scale = max(1.0, float(np.abs(ref).max()))
    err_h = float(np.abs(h0.grad.cpu().numpy() - ref).max())
    print(f"{name}: max |dL/dh0 - reference| = {err_h:.3e} (scale {scale:.3e})")
    assert err_h <= 1e-5 * scale, f"{name}: max |dL/dh0 - reference| = {err_h:.3e}"
    if cost is not None:
        err = float(np.abs(cost.grad.cpu().numpy() - g.grad_cost).max())
        print(f"{name}: max |dL/dcost - reference| = {err:.3e}")
        assert err <= 1e-5 * max(1.0, float(np.abs(g.grad_cost).max())), f"{name}: max |dL/dcost - reference| = {err:.3e}"
        assert torch.equal(h0.grad, cost.grad), "the gradient of heuristic_maps IS the gradient of cost_maps"


# ---- identity sweep: the built-in heuristic handed over as a tensor ---------------------------------------------------------------------
def _random_batch(B, H, W, seed, p=0.2):
    from neural_astar.utils import synthetic as syn
    pr = syn.random_obstacle_maps(B, H, W, p, seed=seed)
    cost = syn.random_costs(B, H, W, seed=seed + 1)
    return [_t(x) for x in (cost, pr.start_maps, pr.goal_maps, pr.map_designs)]


IDENTITY = [(8, 16, 16), (8, 32, 32), (4, 64, 64), (4, 20, 45), (2, 79, 79), (2, 80, 80), (2, 128, 128), (1, 260, 270), (1, 512, 512)]


@pytest.mark.parametrize("g_ratio", [0.5, 0.2])
@pytest.mark.parametrize("shape", IDENTITY, ids=lambda s: f"{s[0]}x{s[1]}x{s[2]}")
def test_builtin_heuristic_as_a_tensor_is_the_default_call(shape, g_ratio):
    _identity(shape, g_ratio)


def test_identity_with_a_misaligned_and_a_strided_heuristic():
    _identity((4, 32, 32), 0.5, view="misaligned")
    _identity((3, 20, 45), 0.5, view="misaligned")
    _identity((4, 32, 32), 0.5, view="strided")


def test_identity_with_the_training_budget():
    _identity((8, 32, 32), 0.5, Tmax=0.25, training=True)
    _identity((2, 96, 96), 0.5, Tmax=0.05, training=True)


def _identity(shape, g_ratio, view=None, Tmax=1.0, training=False):
    from neural_astar import ops
    B, H, W = shape
    cost, s, goal, p = _random_batch(B, H, W, seed=7 * sum(shape) + int(10 * g_ratio))
    h0 = ops.heuristic(goal)
    if view == "misaligned":  # contiguous, but its first element sits 4 bytes past a 16-byte boundary: the scalar loads
        buf = torch.empty(h0.numel() + 1, dtype=torch.float32, device=h0.device)
        buf[1:].copy_(h0.reshape(-1))
        h0 = buf[1:].reshape(h0.shape)
        assert h0.data_ptr() % 16 == 4 and h0.is_contiguous()
    elif view == "strided":  # made contiguous by forward()
        wide = torch.zeros(B, 1, H, 2 * W, dtype=torch.float32, device=h0.device)
        wide[..., ::2] = h0
        h0 = wide[..., ::2]
        assert not h0.is_contiguous()
    max_iters = ops.max_iters_for(W, Tmax, training)
    exact = B > 1 and ops.coupling_possible(g_ratio)
    # the launches themselves: histories, paths, iters, status and the selection log, bit for bit
    a = ops.search_nograd(cost, s, goal, p, g_ratio, max_iters, True, exact=exact)
    b = ops.search_nograd(cost, s, goal, p, g_ratio, max_iters, True, exact=B > 1, heuristic=h0)
    ia = a[2].cpu().numpy()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    la, lb = a[4].cpu().numpy(), b[4].cpu().numpy()
    for i in range(B):
        assert np.array_equal(la[i, :ia[i]], lb[i, :ia[i]]), f"map {i}: selection logs differ"
    # the modules under autograd: same outputs, gradients within the project's bar, and dL/dh0 == dL/dcost
    up = torch.from_numpy(np.random.Generator(np.random.PCG64(5)).standard_normal((B, 1, H, W)).astype(np.float32)).to(_dev())
    c1 = cost.clone().requires_grad_(True)
    m = _module(g_ratio, Tmax, training)
    o1 = m(c1, s, goal, p)
    (o1.histories * up).sum().backward()
    c2 = cost.clone().requires_grad_(True)
    h2 = h0.detach().requires_grad_(True) if view is None else h0
    o2 = m(c2, s, goal, p, heuristic_maps=h2)
    (o2.histories * up).sum().backward()
    assert torch.equal(o1.histories, o2.histories) and torch.equal(o1.paths, o2.paths)
    assert torch.equal(o1.histories[:, 0], a[0]) and torch.equal(o1.paths[:, 0], a[1])
    scale = max(1.0, float(c1.grad.abs().max()))
    err = float((c1.grad - c2.grad).abs().max())
    assert err <= 1e-5 * scale, f"gradients differ by {err:.3e} (scale {scale:.3e})"
    if view is None:
        assert torch.equal(h2.grad, c2.grad)


# ---- random sweep against the numpy restatement -----------------------------------------------------------------------------------------
def _sweep_cases():
    """(name, B, H, W, kind, g_ratio, mask, signed) -- deterministic; LDS sizes with compile-time and runtime dimensions, large-map sizes"""
    cases = []
    lds = [(16, 16), (32, 32), (24, 20), (20, 45), (64, 64), (33, 31)]
    kinds = ["field", "zero", "scaled", "field"]
    i = 0
    for B in (1, 5):
        for (H, W) in lds:
            for mask in (HO.MOORE8, HO.VON_NEUMANN):
                kind = kinds[i % len(kinds)]
                g_ratio = (0.5, 0.2, 0.8)[i % 3]
                cases.append((f"lds{i}", B if (H, W) != (64, 64) else min(B, 2), H, W, kind, g_ratio, mask, i % 2 == 1))
                i += 1
    for B, (H, W), kind, g_ratio, mask, signed in [(1, (80, 80), "field", 0.5, HO.MOORE8, False), (3, (80, 84), "scaled", 0.5, HO.MOORE8, True),
                                                    (3, (96, 100), "field", 0.5, HO.VON_NEUMANN, False), (4, (90, 80), "field", 0.2, HO.MOORE8, False),
                                                    (2, (100, 96), "zero", 0.5, HO.MOORE8, True), (3, (88, 88), "field", 0.5, HO.MOORE8, False)]:
        cases.append((f"large{i}", B, H, W, kind, g_ratio, mask, signed))
        i += 1
    # batches of random fields at g_ratio 0.5: the class in which a finished map leaves its fixed point (about 1 map in 4 does)
    for (H, W) in [(24, 24), (32, 32), (16, 16), (20, 45), (28, 36), (80, 80), (82, 80), (80, 90), (84, 84)]:
        cases.append((f"batch{i}", 6 if H * W < 6400 else 4, H, W, "field", 0.5, HO.MOORE8, False))
        i += 1
    # von Neumann moves through denser obstacles: some maps have no route
    for (H, W) in [(16, 16), (32, 32), (20, 45)]:
        cases.append((f"dense{i}", 4, H, W, "zero" if H == 16 else "field", 0.5, HO.VON_NEUMANN, False))
        i += 1
    return cases


def _sweep_inputs(case):
    from neural_astar.utils import synthetic as syn
    name, B, H, W, kind, g_ratio, mask, signed = case
    seed = 1000 + sum(ord(ch) for ch in name) + 13 * H + W
    rng = np.random.Generator(np.random.PCG64(seed))
    pr = syn.random_obstacle_maps(B, H, W, 0.4 if name.startswith("dense") else 0.15 if mask == HO.VON_NEUMANN else 0.25, seed=seed)
    cost = rng.random((B, 1, H, W)).astype(np.float32)
    if signed:
        cost = (cost * np.float32(1.3) - np.float32(0.3)).astype(np.float32)
    if kind == "field":
        h0 = (rng.random((B, 1, H, W)) * 5.0 - 1.0).astype(np.float32)
    elif kind == "zero":
        h0 = np.zeros((B, 1, H, W), np.float32)
    else:  # a multiple of the Chebyshev distance: weighted search
        gi = pr.goal_maps.reshape(B, -1).argmax(1)
        rr, cc = np.mgrid[0:H, 0:W]
        h0 = np.stack([np.float32(1.7) * np.maximum(np.abs(rr - g // W), np.abs(cc - g % W)).astype(np.float32) for g in gi])[:, None]
    return cost, pr.start_maps, pr.goal_maps, pr.map_designs, h0.astype(np.float32)


def test_random_sweep_against_the_numpy_restatement():
    counts = dict(lds_pow2=0, lds_runtime=0, large=0, coupled=0, coupled_large=0, von_neumann=0, signed=0, single=0, unsolvable=0, maps=0)
    for case in _sweep_cases():
        name, B, H, W, kind, g_ratio, mask, signed = case
        cost, start, goal, maps, h0 = _sweep_inputs(case)
        o = HO.search(cost, start, goal, maps, h0, g_ratio, W * W, mask, lockstep=B > 1)
        m = _module(g_ratio, mask=mask, check_solvable=False)
        out = m(_t(cost), _t(start), _t(goal), _t(maps), heuristic_maps=_t(h0))
        status = m.last_status.cpu().numpy()
        assert np.array_equal(status, o.status), f"{name}: status {status} vs {o.status}"  # an unsolvable map carries the status in both
        ok = o.status == 0
        hist, paths, iters = out.histories[:, 0].cpu().numpy(), out.paths[:, 0].cpu().numpy(), m.last_iters.cpu().numpy()
        assert np.array_equal(hist[ok], o.histories[ok]), f"{name}: histories"
        assert np.array_equal(paths[ok], o.paths[ok]), f"{name}: paths"
        if ok.any():
            assert int(iters[ok].max()) - 1 == o.t_batch, f"{name}: t_batch"
        counts["maps"] += B
        counts["unsolvable"] += int((~ok).sum())
        counts["single"] += B == 1
        counts["von_neumann"] += mask == HO.VON_NEUMANN
        counts["signed"] += bool(signed)
        counts["large" if H * W >= 6400 else ("lds_pow2" if H == W and W in (16, 32, 64) else "lds_runtime")] += 1
        if B > 1:
            alone = HO.search(cost, start, goal, maps, h0, g_ratio, W * W, mask, lockstep=False)
            left = int(any(not np.array_equal(alone.histories[b], o.histories[b]) for b in range(B) if ok[b]))
            counts["coupled"] += left
            counts["coupled_large"] += left if H * W >= 6400 else 0
    print("random sweep:", counts)
    assert counts["lds_pow2"] >= 12 and counts["lds_runtime"] >= 12 and counts["large"] >= 8
    assert counts["coupled"] >= 4 and counts["coupled_large"] >= 1, "the exact pipeline must be exercised: batches in which a map leaves its fixed point"
    assert counts["von_neumann"] >= 12 and counts["signed"] >= 12 and counts["single"] >= 12
    assert counts["unsolvable"] >= 3 and counts["maps"] - counts["unsolvable"] >= 100


# ---- a NaN / an infinite value in one map's heuristic ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape, value", [((4, 32, 32), float("nan")), ((4, 20, 45), float("inf")), ((3, 96, 96), float("nan")), ((3, 96, 96), float("-inf"))],
                         ids=["lds-nan", "lds-inf", "large-nan", "large-neg-inf"])
def test_a_non_finite_heuristic_is_reported_for_its_map_and_the_others_are_searched(shape, value):
    from neural_astar import ops
    B, H, W = shape
    cost, s, goal, p = _random_batch(B, H, W, seed=99 + H)
    h0 = ops.heuristic(goal).clone()
    h0[1, 0, H - 1, W - 2] = value  # (far from the first cells a load loop looks at)
    m = _module(check_solvable=True)
    with pytest.raises(ValueError, match="non-finite heuristic") as e:
        m(cost, s, goal, p, heuristic_maps=h0)
    assert "[1]" in str(e.value)
    m = _module(check_solvable=False)
    out = m(cost, s, goal, p, heuristic_maps=h0)
    status = m.last_status.cpu().numpy()
    assert status.tolist() == [0, ops.STATUS_BAD_HEURISTIC] + [0] * (B - 2)
    keep = [0] + list(range(2, B))
    ref = _module(check_solvable=False)(cost[keep], s[keep], goal[keep], p[keep])  # the others as a batch of their own, default heuristic
    assert torch.equal(out.histories[keep], ref.histories) and torch.equal(out.paths[keep], ref.paths)
    assert out.histories[1].sum() == 0
