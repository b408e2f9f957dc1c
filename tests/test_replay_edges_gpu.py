"""GPU tests (-m gpu) of the replay backward (nastar_backward_replay*, csrc/nastar_backward_replay.hip.h, nastar_backward_replay_asm.hip.h,
backward_replay_impl in csrc/nastar_capi.hip) on degenerate and batch-coupled problems: searches of one or two steps, budgets that end at
or one step before the goal, maps smaller than a wavefront -- on every replay route.  The problems, the oracle's literal reverse mode
and the bars are those of tests/replay_edges.py (tests/test_replay_edges.py checks, without a GPU, that the oracle alone meets what is
relied on here and that the shared checker refuses a dropped `extra` term, a cell off by 1e-4 of its map's scale and a stray write).

What the kernels must deliver, per MAP and not per batch: 1e-5 * max(1, max|ref_b|), the route's measured relative bar wherever the
map has a gradient, exactly 0.0 outside the cells the search opened, an output without an unwritten cell, and no byte outside the output
and the nastar_backward_workspace_bytes() bytes of workspace."""
import concurrent.futures
import functools
import itertools
import os

import numpy as np
import pytest
import torch

import replay_edges as R

pytestmark = pytest.mark.gpu

GUARD = 4096      # bytes in front of and behind the carved output and workspace
SENTINEL = 0xA5
CASES = list(itertools.product(R.SHAPES, R.VARIANTS))
MEASURED = []     # (route, case, map, relative error) of every map with a gradient: printed per test, summarised by the last test


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).to(_dev())  # (a copy: the shared cases are read-only arrays)


def _sync():
    """wait for the device; a HIP error ends the session -- nothing more is started on a device that faulted"""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"HIP error, session ended: {e}", returncode=3)


def _misaligned(t):
    """the same values in a contiguous view 4 bytes past a 16-byte boundary (as tests/test_heuristic_maps_gpu.py builds one)"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:].copy_(t.reshape(-1))
    out = buf[1:].reshape(t.shape)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


@pytest.fixture(scope="module", autouse=True)
def _oracle_answers():
    """every case's oracle run, several at a time (the calls release the GIL; g_ratio 1 on the largest maps is a 700-step dense run)"""
    R.case("1x1", "u01")
    with concurrent.futures.ThreadPoolExecutor(max(1, min(8, (os.cpu_count() or 2) // 2))) as pool:
        list(pool.map(lambda sv: R.case(sv[0], "u01") and R.case(*sv), CASES))


def _inputs(c):
    cost, s, g, m = (_t(x[:, 0]) for x in (c.cost, c.s, c.g, c.m))
    return (_misaligned(cost) if c.misaligned else cost), s, g, m


def _search(c):
    """the forward with a selection log, equal to the oracle's state machine -> (inputs, sel_log, iters)"""
    from neural_astar import ops
    cost, s, g, m = _inputs(c)
    hist, paths, iters, status, log = ops.search_nograd(cost, s, g, m, c.gr, c.T, want_log=True)
    _sync()
    what = (c.shape, c.variant)
    assert np.array_equal(hist.cpu().numpy(), c.fwd.histories) and np.array_equal(paths.cpu().numpy(), c.fwd.paths), what
    assert np.array_equal(iters.cpu().numpy(), c.fwd.iters) and not status.cpu().numpy().any(), what
    lg = log.cpu().numpy()
    assert all(np.array_equal(lg[b, :c.fwd.iters[b]], c.fwd.sel_log[b, :c.fwd.iters[b]]) for b in range(3)), what
    return (cost, s, g, m), log, iters


def _replay_raw(maps, log, iters, up, gr, T, t_batch, what):
    """nastar_backward_replay straight through the C ABI: grad_cost_out carved out of a NaN-filled buffer, the workspace -- exactly
    nastar_backward_workspace_bytes() bytes -- out of a 0xA5-filled one, GUARD bytes either side of both.  Asserts rc 0 and untouched
    guards -> grad_cost [B, H, W] as numpy"""
    from neural_astar import _native
    lib = _native.load()
    dev = _dev()
    cost, s, g, m = maps
    B, H, W = s.shape
    n = B * H * W
    gw = GUARD // 4
    out = torch.full((gw + n + gw,), float("nan"), dtype=torch.float32, device=dev)
    nbytes = int(lib.nastar_backward_workspace_bytes(B, H, W, T))
    assert nbytes > 0
    ws = torch.full((GUARD + nbytes + GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
    assert out.data_ptr() % 16 == 0 and ws.data_ptr() % 16 == 0
    nan_bits = out[:1].view(torch.int32).item()
    tb = None if t_batch is None else torch.tensor([t_batch], dtype=torch.int32, device=dev)
    rc = lib.nastar_backward_replay(up.data_ptr(), cost.data_ptr(), s.data_ptr(), g.data_ptr(), m.data_ptr(), log.data_ptr(), B, H, W,
                                    float(gr), int(T), iters.data_ptr(), None if tb is None else tb.data_ptr(), out.data_ptr() + GUARD,
                                    ws.data_ptr() + GUARD, nbytes, 0, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, (what, rc)
    _sync()
    bits = out.view(torch.int32)
    assert bool((bits[:gw] == nan_bits).all()), f"{what}: floats in FRONT of grad_cost_out were written"
    assert bool((bits[gw + n:] == nan_bits).all()), f"{what}: floats BEHIND grad_cost_out were written"
    assert bool((ws[:GUARD] == SENTINEL).all()), f"{what}: bytes in FRONT of the workspace were written"
    assert bool((ws[GUARD + nbytes:] == SENTINEL).all()), f"{what}: bytes BEHIND the workspace's {nbytes} bytes were written"
    return out[gw:gw + n].reshape(B, H, W).cpu().numpy()


@functools.lru_cache(maxsize=None)
def _abi_gradient(shape, variant):
    """item 1's run of one case, shared with the module-path test: the full batch, t_batch = max(iters) - 1"""
    c = R.case(shape, variant)
    maps, log, iters = _search(c)
    got = _replay_raw(maps, log, iters, _t(c.up[:, 0]), c.gr, c.T, int(c.fwd.iters.max()) - 1, f"{shape} {variant}")
    got.setflags(write=False)
    return got


# ---- 1 + 2: every shape x variant through the C ABI, per-map bars ---------------------------------------------------------------------------

@pytest.mark.parametrize("shape,variant", CASES)
def test_replay_through_the_c_abi(shape, variant):
    c = R.case(shape, variant)
    got = _abi_gradient(shape, variant)
    R.check_grad(got, c.ref, c.opened, c.route, f"{shape} {variant}", MEASURED)
    if variant in R.EXACTLY_ZERO:
        assert not got.any(), f"{shape} {variant}: the gradient must be exactly zero everywhere, max|got| = {np.abs(got).max():.3e}"


# ---- 3: t_batch semantics -------------------------------------------------------------------------------------------------------------------

T_BATCH_SHAPES = ["32x32", "20x45", "110x110"]


@pytest.mark.parametrize("shape", T_BATCH_SHAPES)
def test_t_batch_null_is_every_map_as_its_own_batch(shape):
    c = R.case(shape, "u01")
    maps, log, iters = _search(c)
    got = _replay_raw(maps, log, iters, _t(c.up[:, 0]), c.gr, c.T, None, f"{shape} t_batch NULL")
    R.check_grad(got, R.alone(c), c.opened, c.route, f"{shape} t_batch NULL", MEASURED)
    assert not got[0].any(), f"{shape}: the start == goal map on its own has no gradient, max|got| = {np.abs(got[0]).max():.3e}"


@pytest.mark.parametrize("shape", T_BATCH_SHAPES)
def test_a_shard_with_the_whole_batchs_t_batch_equals_the_whole_batchs_rows(shape):
    """the multi-GPU contract of include/nastar.h: maps 0 and 1 replayed as B = 2 with t_batch = max(iters) - 1 over ALL three maps"""
    c = R.case(shape, "u01")
    maps, log, iters = _search(c)
    shard = tuple(x[:2].contiguous() for x in maps)
    got = _replay_raw(shard, log[:2].contiguous(), iters[:2].contiguous(), _t(c.up[:2, 0]), c.gr, c.T, int(c.fwd.iters.max()) - 1,
                      f"{shape} shard")
    R.check_grad(got, c.ref[:2], c.opened[:2], c.route, f"{shape} shard of maps 0, 1", MEASURED)


@pytest.mark.parametrize("shape", T_BATCH_SHAPES)
def test_two_start_is_goal_maps_give_zeros_fully_written(shape):
    from neural_astar import ops
    c = R.case(shape, "u01")
    cost, s, g, m = (_t(np.repeat(x[:1, 0], 2, 0)) for x in (c.cost, c.s, c.g, c.m))
    _, _, iters, status, log = ops.search_nograd(cost, s, g, m, c.gr, c.T, want_log=True)
    _sync()
    assert iters.tolist() == [1, 1] and status.tolist() == [0, 0]
    up = _t(np.repeat(c.up[:1, 0], 2, 0))
    got = _replay_raw((cost, s, g, m), log, iters, up, c.gr, c.T, 0, f"{shape} two start == goal maps")  # (no NaN left: fully written)
    assert not np.isnan(got).any() and not got.any(), f"{shape}: max|got| = {np.nanmax(np.abs(got)):.3e}"


# ---- 4: placement ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["32x32", "64x64"])
def test_reversed_placement_is_bit_identical(shape):
    from neural_astar import ops
    c = R.case(shape, "u01")
    (cost, s, g, m), log, iters = _search(c)
    up = _t(c.up[:, 0])
    tb = torch.tensor([int(c.fwd.iters.max()) - 1], dtype=torch.int32, device=_dev())
    natural = ops.astar_backward_replay(up, cost, s, g, m, log, c.gr, c.T, iters, tb)
    order = torch.tensor([2, 1, 0], dtype=torch.int32, device=_dev())
    placed = ops.astar_backward_replay(up, cost, s, g, m, log, c.gr, c.T, iters, tb, order)
    _sync()
    natural, placed = natural.cpu().numpy(), placed.cpu().numpy()
    assert np.array_equal(natural.view(np.uint32), placed.view(np.uint32))
    R.check_grad(natural, c.ref, c.opened, c.route, f"{shape} through the op", MEASURED)


# ---- 5: the fused L1 form -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("shape", ["32x32", "16x16", "20x45", "110x110"])
def test_fused_l1_loss_and_its_gradient(shape, scaled):
    """ops.astar_l1_loss: the search, mean|histories - opt_trajs| and, in the backward, sign(h - t) / numel formed inside the replay
    kernel.  Random 0/1 targets; map 1 whole and every second row of the others equal the histories, so sign(0) = 0 occurs.  `scaled`:
    the loss times numel before .backward() -- the upstream values are then +-1 and every map's gradient is large enough for the
    relative bar (the plain mean's gradients are numel times smaller: the absolute bar alone would let almost anything pass)."""
    from neural_astar import ops
    from oracle import oracle as O
    c = R.case(shape, "u01")
    cost, s, g, m = _inputs(c)
    rng = np.random.default_rng(c.H * 1000 + c.W)
    opt = (rng.random(c.fwd.histories.shape) < 0.5).astype(np.float32)
    opt[1] = c.fwd.histories[1]
    opt[:, ::2] = c.fwd.histories[:, ::2]
    cost = cost.clone().requires_grad_(True)
    loss, hist, _, iters, status = ops.astar_l1_loss(cost, s, g, m, _t(opt), c.gr, c.T)
    numel = opt.size
    (loss * numel if scaled else loss).backward()
    _sync()
    assert np.array_equal(hist.cpu().numpy(), c.fwd.histories) and np.array_equal(iters.cpu().numpy(), c.fwd.iters)
    want = np.abs(c.fwd.histories.astype(np.float64) - opt).mean()
    assert abs(float(loss.detach()) - want) <= 1e-6, (float(loss.detach()), want)
    sign = np.sign(c.fwd.histories - opt).astype(np.float32)
    assert (sign == 0).any() and (sign > 0).any() and (sign < 0).any()
    up = sign if scaled else (sign * np.float32(1.0 / numel)).astype(np.float32)
    ref = O.backward(up[:, None], c.cost, c.s, c.g, c.m, c.gr, c.T)
    R.check_grad(cost.grad.cpu().numpy(), ref, c.opened, c.route, f"{shape} fused L1{' x numel' if scaled else ''}", MEASURED)


# ---- 6: the module path ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["u01", "T3"])
@pytest.mark.parametrize("shape", ["32x32", "2x2"])
def test_module_under_autograd_equals_the_c_abi_result(shape, variant):
    """DifferentiableAstar in eval mode (the budget W * W) and in training mode with the Tmax that gives T = 3: the same launch with the same
    arguments as item 1 made through the C ABI -- the same bits"""
    from neural_astar.planner.differentiable_astar import DifferentiableAstar
    c = R.case(shape, variant)
    train = variant == "T3"
    da = DifferentiableAstar(c.gr, 3.5 / (c.W * c.W) if train else 1.0).to(_dev()).train(train)
    cost = _t(c.cost).requires_grad_(True)
    out = da(cost, _t(c.s), _t(c.g), _t(c.m))
    (out.histories * _t(c.up)).sum().backward()
    _sync()
    assert np.array_equal(out.histories[:, 0].detach().cpu().numpy(), c.fwd.histories) and np.array_equal(da.last_iters.cpu().numpy(), c.fwd.iters)
    got = cost.grad[:, 0].cpu().numpy()
    R.check_grad(got, c.ref, c.opened, c.route, f"{shape} {variant} module", MEASURED)
    assert np.array_equal(got.view(np.uint32), _abi_gradient(shape, variant).view(np.uint32))


@pytest.mark.parametrize("H,W", [(40, 1), (1, 40), (2, 2)])
def test_heuristic_kernel_on_one_column_and_one_row_maps(H, W):
    """nastar_heuristic shares the search kernels' row-by-magic-multiply, which had no magic for W = 1 (every cell in row 0): the 40x1 T3
    case above is the search, this is the stand-alone kernel -- bit-exact with the oracle's get_heuristic"""
    from neural_astar import ops
    from oracle import oracle as O
    cells = [(H - 1, W - 1), (H // 2, W // 2), (0, 0)]
    goal = np.zeros((3, H, W), np.float32)
    for b, rc in enumerate(cells):
        goal[b][rc] = 1
    h = ops.heuristic(_t(goal)).cpu().numpy()
    for b, (r, c) in enumerate(cells):
        assert np.array_equal(h[b].view(np.uint32), O.heuristic(H, W, r, c).view(np.uint32)), (H, W, r, c)


def test_zz_measured_relative_errors_per_route():
    """(runs last in this file) the largest per-map relative error of every route this session measured -- the figures of the table in
    tests/replay_edges.py -- and that no route went unmeasured"""
    worst = {}
    for route, what, b, rel in MEASURED:
        if rel >= worst.get(route, (-1.0,))[0]:
            worst[route] = (rel, what, b)
    for route in sorted(worst):
        rel, what, b = worst[route]
        print(f"replay_edges worst route={route} rel={rel:.3e} bar={R.rel_bar(route):.3e} at {what} map {b}")
    if len({w for _, w, _, _ in MEASURED}) >= len(CASES) // 2:  # (the whole file ran, not a selection of it)
        assert set(worst) == {r for r in (R.SHAPES[s][4] for s in R.SHAPES)}
