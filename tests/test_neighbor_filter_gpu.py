"""GPU (-m gpu): DifferentiableAstar.neighbor_filter on the kernels against the reference run with the same filter
(tests/golden/neighbors/, tools/gen_golden_neighbors.py): forward bit-exact, selection logs, gradients, filter changes and refusals."""
import copy

import numpy as np
import pytest
import torch

import neighbor_golden as NG

pytestmark = pytest.mark.gpu

VN = [[0, 1, 0], [1, 0, 1], [0, 1, 0]]
FORWARD = [n for n in NG.names() if not n.startswith("grad_")]
GRAD = [n for n in NG.names() if n.startswith("grad_")]


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _module(g, check_solvable=True):
    from neural_astar.planner.differentiable_astar import DifferentiableAstar
    m = DifferentiableAstar(g_ratio=g.g_ratio, Tmax=g.Tmax, check_solvable=check_solvable).to(_dev())
    with torch.no_grad():
        m.neighbor_filter.copy_(_t(g.filter).reshape(1, 1, 3, 3))
    m.train(g.training)
    return m


@pytest.mark.parametrize("grad", [False, True])
@pytest.mark.parametrize("check", [True, "deferred", False])
@pytest.mark.parametrize("name", FORWARD)
def test_forward_matches_reference(name, check, grad):
    g = NG.load(name)
    m = _module(g, check)
    cost = _t(g.cost_maps).requires_grad_(grad)
    with torch.set_grad_enabled(grad):
        out = m(cost, _t(g.start_maps), _t(g.goal_maps), _t(g.map_designs))
    if check == "deferred":
        m.raise_if_unsolvable()
    assert np.array_equal(out.histories.detach().cpu().numpy(), g.histories), f"{name}: histories differ from the reference"
    assert np.array_equal(out.paths.cpu().numpy(), g.paths), f"{name}: paths differ from the reference"
    assert int(m.last_iters.max()) - 1 == g.t_batch  # the reference's loop index at its break


@pytest.mark.parametrize("name", FORWARD)
def test_selection_logs_match_reference(name):
    from neural_astar import ops
    g = NG.load(name)
    cost, s, goal, p = (_t(x)[:, 0] for x in (g.cost_maps, g.start_maps, g.goal_maps, g.map_designs))
    exact = cost.shape[0] > 1 and ops.coupling_possible(g.g_ratio)
    hist, paths, iters, status, log = torch.ops.nastar.astar_forward(cost, s, goal, p, g.g_ratio, g.max_iters, True, 0, 0, exact, NG.mask_of(g.filter))
    assert (status == 0).all()
    iters, log = iters.cpu().numpy(), log.cpu().numpy()
    for b in range(cost.shape[0]):
        n = int(iters[b])
        assert np.array_equal(log[b, :n], g.sel_log[b, :n]), f"{name}: map {b} selects differently from the reference"
    assert np.array_equal(hist.cpu().numpy(), g.histories[:, 0])


def test_store_intermediate_results_equal_the_references():
    g = NG.load("fixture64_vn_g050")
    m = _module(g)
    out = m(_t(g.cost_maps), _t(g.start_maps), _t(g.goal_maps), _t(g.map_designs), store_intermediate_results=True)
    ir = out.intermediate_results
    assert len(ir) == g.inter_hist.shape[0] == g.t_batch + 2
    for t in (0, 1, 2, len(ir) // 2, len(ir) - 2, len(ir) - 1):
        assert np.array_equal(ir[t]["histories"].cpu().numpy(), g.inter_hist[t]), t
        assert np.array_equal(ir[t]["paths"].cpu().numpy().astype(np.float32), g.inter_path[t]), t


@pytest.mark.parametrize("name", GRAD)
def test_l1_gradients_match_reference(name):
    g = NG.load(name)
    m = _module(g)
    cost = _t(g.cost_maps).requires_grad_(True)
    out = m(cost, _t(g.start_maps), _t(g.goal_maps), _t(g.map_designs))
    assert np.array_equal(out.histories.detach().cpu().numpy(), g.histories)
    torch.nn.L1Loss()(out.histories, _t(g.target)).backward()
    err = float(np.abs(cost.grad.cpu().numpy() - g.grad_cost).max())
    assert err <= 1e-5 * max(1.0, float(np.abs(g.grad_cost).max())), f"{name}: max |grad - reference| = {err:.3e}"


def _random_batch(B, H, W, seed):
    from neural_astar.utils import synthetic as syn
    pr = syn.random_obstacle_maps(B, H, W, 0.2, seed=seed)
    cost = syn.random_costs(B, H, W, seed=seed + 1)
    return [_t(x) for x in (cost, pr.start_maps, pr.goal_maps, pr.map_designs)]


def test_switching_filters_between_calls_is_honoured():
    from neural_astar.planner.differentiable_astar import DifferentiableAstar
    g = NG.load("fixture64_vn_g050")
    x = [_t(a) for a in (g.cost_maps, g.start_maps, g.goal_maps, g.map_designs)]
    m = DifferentiableAstar().to(_dev()).eval()
    moore = m(*x).histories.sum().item()
    assert moore == 1169
    for filt, want in ((VN, 3395), ([[1, 1, 1], [1, 0, 1], [1, 1, 1]], 1169), (VN, 3395)):
        with torch.no_grad():
            m.neighbor_filter.copy_(torch.tensor(filt, dtype=torch.float32, device=_dev()).reshape(1, 1, 3, 3))
        assert m(*x).histories.sum().item() == want
    # a checkpoint that carries a von Neumann filter
    m2 = DifferentiableAstar().to(_dev()).eval()
    sd = m2.state_dict()
    sd["neighbor_filter"] = torch.tensor(VN, dtype=torch.float32).reshape(1, 1, 3, 3)
    m2.load_state_dict(sd)
    out = m2(*x)
    assert np.array_equal(out.histories.cpu().numpy(), g.histories) and np.array_equal(out.paths.cpu().numpy(), g.paths)


@pytest.mark.parametrize("shape", [(64, 32, 32), (8, 64, 64), (4, 20, 45), (2, 96, 96)])
def test_moore8_written_back_equals_the_untouched_default(shape):
    from neural_astar.planner.differentiable_astar import DifferentiableAstar
    x = _random_batch(*shape, seed=sum(shape))
    ref = DifferentiableAstar(check_solvable=False).to(_dev()).eval()
    m = DifferentiableAstar(check_solvable=False).to(_dev()).eval()  # (some of these maps are 8-connected only: von Neumann cannot solve them)
    with torch.no_grad():
        m.neighbor_filter.copy_(torch.tensor(VN, dtype=torch.float32, device=_dev()).reshape(1, 1, 3, 3))
    m(*x)
    with torch.no_grad():
        m.neighbor_filter.fill_(1.0)
        m.neighbor_filter[0, 0, 1, 1] = 0
    a, b = ref(*x), m(*x)
    assert np.array_equal(a.histories.cpu().numpy(), b.histories.cpu().numpy())
    assert np.array_equal(a.paths.cpu().numpy(), b.paths.cpu().numpy())


@pytest.mark.parametrize("shape", [(64, 32, 32), (8, 64, 64), (4, 20, 45), (2, 96, 96)])
def test_masked_kernels_with_the_moore8_mask_equal_the_default_kernels(shape):
    """nastar_forward_ex_masked runs the masked instantiations for every mask: with 0x1EF they must compute what the default kernels do"""
    from neural_astar import ops
    cost, s, g, p = (t[:, 0] for t in _random_batch(*shape, seed=3 * sum(shape)))
    W = shape[-1]
    a = ops.search_nograd(cost, s, g, p, 0.5, W * W, True)
    b = ops.search_nograd(cost, s, g, p, 0.5, W * W, True, neighbor_mask=ops.NEIGHBORS_MOORE8)
    for x, y in zip(a[:4], b[:4]):
        assert torch.equal(x, y)
    it = a[2].cpu().numpy()
    la, lb = a[4].cpu().numpy(), b[4].cpu().numpy()
    for i in range(shape[0]):
        assert np.array_equal(la[i, :it[i]], lb[i, :it[i]])


def test_unsolvable_under_the_neighbourhood_goes_through_the_unsolvable_protocol():
    from neural_astar.planner.differentiable_astar import DifferentiableAstar, UnsolvableMapError
    m = torch.ones(2, 1, 8, 8, device=_dev())
    m[:, :, 3:5, :] = 0  # a wall two rows thick ...
    m[:, :, 3, 4] = 1
    m[0, :, 4, 4] = 1  # ... map 0: a straight gap
    m[1, :, 4, 5] = 1  # ... map 1: only a diagonal step crosses it
    s = torch.zeros_like(m)
    s[:, :, 0, 0] = 1
    gl = torch.zeros_like(m)
    gl[:, :, 7, 7] = 1
    da = DifferentiableAstar().to(_dev()).eval()
    da(m, s, gl, m)  # Moore-8: both solvable
    with torch.no_grad():
        da.neighbor_filter.copy_(torch.tensor(VN, dtype=torch.float32, device=_dev()).reshape(1, 1, 3, 3))
    with pytest.raises(UnsolvableMapError):
        da(m, s, gl, m)
    assert da.last_status.cpu().tolist() == [0, 3]
    with torch.no_grad():
        da.neighbor_filter.zero_()  # the all-zero filter is legal: nothing but start == goal is solvable
    with pytest.raises(UnsolvableMapError):
        da(m, s, gl, m)
    out = da(m, s, s, m)
    assert (da.last_status == 0).all() and out.paths.sum().item() == 2


def test_routes_that_cannot_honour_a_filter_refuse_and_the_rest_honour_it():
    from neural_astar.parallel import InFlightPlanner
    from neural_astar.planner import VanillaAstar
    from neural_astar.utils.training import fused_l1_step
    g = NG.load("fixture64_vn_g050")
    maps, s, gl = (_t(a) for a in (g.map_designs, g.start_maps, g.goal_maps))
    planner = VanillaAstar().to(_dev()).eval()
    with torch.no_grad():
        planner.astar.neighbor_filter.copy_(_t(g.filter).reshape(1, 1, 3, 3))
    out = planner(maps, s, gl)  # VanillaAstar.forward: cost == obstacle map (unit-cost layout is skipped for a filter)
    assert np.array_equal(out.histories.cpu().numpy(), g.histories)
    planner.astar.unit_cost = True
    assert np.array_equal(planner(maps, s, gl).histories.cpu().numpy(), g.histories)
    with pytest.raises(NotImplementedError, match="neighbor_filter"):
        InFlightPlanner(planner).submit(maps, s, gl)
    loss, o2 = fused_l1_step(planner, maps, s, gl, torch.zeros_like(maps))  # honoured (the planner's own forward + L1Loss)
    assert np.array_equal(o2.histories.detach().cpu().numpy(), g.histories)
    assert abs(loss.item() - g.histories.mean()) < 1e-6
    with torch.no_grad():
        planner.astar.neighbor_filter.mul_(0.5)
    with pytest.raises(NotImplementedError, match="neighbor_filter"):
        planner(maps, s, gl)
    cp = copy.deepcopy(planner)  # (module state survives a copy; the cache is rebuilt)
    with pytest.raises(NotImplementedError, match="neighbor_filter"):
        cp(maps, s, gl)


def test_validation_step_compares_against_a_moore8_vanilla_astar():
    """PlannerModule.validation_step with a von Neumann planner: the baseline is the reference's default VanillaAstar() (Moore-8), searched
    apart from the planner -- the metrics equal a planner call plus a default VanillaAstar call"""
    from types import SimpleNamespace
    from neural_astar.planner import NeuralAstar, VanillaAstar
    from neural_astar.utils import synthetic as syn
    from neural_astar.utils.metrics import validation_metrics
    from neural_astar.utils.training import PlannerModule
    dev = _dev()
    torch.manual_seed(0)
    pr = syn.random_obstacle_maps(16, 32, 32, 0.1, seed=91)
    m, s, g = (_t(x) for x in pr)
    planner = NeuralAstar(encoder_arch="CNN").to(dev).eval()
    planner.astar.check_solvable = False  # (a few of these maps may need a diagonal step)
    with torch.no_grad():
        planner.astar.neighbor_filter.copy_(torch.tensor(VN, dtype=torch.float32, device=dev).reshape(1, 1, 3, 3))
    mod = PlannerModule(planner, SimpleNamespace(params=SimpleNamespace(lr=1e-3))).to(dev).eval()
    logged = {}
    mod.log = lambda name, value, *a, **k: logged.__setitem__(name, value)
    with torch.no_grad():
        mod.validation_step((m, s, g, torch.zeros_like(m)), 0)
        out = planner(m, s, g)
        va = VanillaAstar().to(dev).eval()
        va.astar.check_solvable = False
        va_out = va(m, s, g)
        vn_va = VanillaAstar().to(dev).eval()
        vn_va.astar.check_solvable = False
        vn_va.astar.neighbor_filter.copy_(planner.astar.neighbor_filter)
        vn_out = vn_va(m, s, g)
    assert not torch.equal(va_out.histories, vn_out.histories)  # the two baselines differ on these maps: the test can tell them apart
    want = validation_metrics(out, va_out)
    for k in ("p_opt", "p_exp", "h_mean"):
        assert float(logged[f"metrics/{k}"]) == float(getattr(want, k)), k


def test_captured_graph_keeps_the_mask_and_a_changed_filter_refuses_capture(monkeypatch):
    from neural_astar.planner import VanillaAstar
    from neural_astar.utils import synthetic as syn
    dev = _dev()
    g0 = NG.load("rand32_asym_g050")
    g1 = NG.load("fixture64_vn_g050")
    va = VanillaAstar().to(dev).eval()
    va.astar.check_solvable = "deferred"
    with torch.no_grad():
        va.astar.neighbor_filter.copy_(_t(g0.filter).reshape(1, 1, 3, 3))
    maps, s, gl = (_t(x).clone() for x in (g0.map_designs, g0.start_maps, g0.goal_maps))
    with torch.no_grad():
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(2):  # warm-up on the capture stream; the mask is read (and cached) here
                va(maps, s, gl)
        torch.cuda.current_stream(dev).wait_stream(side)
        va.astar.raise_if_unsolvable()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = va(maps, s, gl)
        graph.replay()
        torch.cuda.synchronize()
    assert np.array_equal(out.histories.cpu().numpy(), g0.histories) and np.array_equal(out.paths.cpu().numpy(), g0.paths)
    # a filter changed after its mask was cached cannot be read inside a capture: the call refuses instead of searching the old neighbourhood
    with torch.no_grad():
        va.astar.neighbor_filter.copy_(_t(g1.filter).reshape(1, 1, 3, 3))
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="neighbor_filter changed"):
        va.astar.neighbor_mask()
    monkeypatch.undo()
    assert va.astar.neighbor_mask() == NG.mask_of(g1.filter)  # outside a capture it is simply read again
