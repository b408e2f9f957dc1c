"""GPU (-m gpu): the masked kernels (DifferentiableAstar.neighbor_filter; nastar_forward_ex_masked, nastar_forward_batchloop_finish_masked,
nastar_backward_replay_ordered_masked) against the oracle's masked restatements (oracle/nastar_oracle.c *_masked, pinned on the CPU by
tests/test_oracle_neighbors.py): randomised sweeps over masks, shapes and inputs that reach every masked kernel instantiation
(tools/fuzz_parity.py run_masked / run_backward_masked / run_module_masked; `python tools/fuzz_parity.py masked <seed> <n>` runs long
sweeps), and named cases per route -- one ray per filter cell, forced detours, maps above 65,519 cells, placement and packed outputs."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import fuzz_parity as FP  # noqa: E402

# one shape per forward route (fuzz_parity.masked_route): compile-time 16x16 / 32x32 / 64x64, runtime sizes (20x24: one chunk per lane;
# 33x31: scalar loads, IEEE division), the hybrid large-map kernel with fast (96x96) and IEEE (80x80) division
RAY_SHAPES = [(16, 16), (32, 32), (64, 64), (20, 24), (33, 31), (96, 96), (80, 80)]


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _onehot(idx, H, W):
    a = np.zeros((len(idx), 1, H, W), np.float32)
    a.reshape(len(idx), -1)[np.arange(len(idx)), idx] = 1.0
    return a


def _search(cost, start, goal, maps, mask, g_ratio=0.5, want_log=True):
    from neural_astar import ops
    W = maps.shape[-1]
    out = ops.search_nograd(_t(cost[:, 0]), _t(start[:, 0]), _t(goal[:, 0]), _t(maps[:, 0]), g_ratio, W * W, want_log=want_log, neighbor_mask=mask)
    torch.cuda.synchronize()
    return out


def test_masked_search_sweep_reaches_every_kernel_and_matches_the_oracle():
    stats, bad = FP.run_masked(seed=7, N=100, verbose=False)
    print("run_masked per route:", stats)
    assert not bad, bad[:5]
    for route in FP.ROUTE_SHAPES:
        assert stats.get(route, 0) >= 2, (route, stats)
    assert stats["lds_rt_scalar_fastdiv"] >= 4  # (the misaligned 32x32 views land here too)
    assert stats.get("with_log", 0) >= 25 and stats.get("placed", 0) >= 20, stats


def test_masked_replay_backward_sweep_matches_the_oracle_reverse_mode():
    stats, bad = FP.run_backward_masked(seed=13, N=22, verbose=False)
    print("run_backward_masked per route:", stats)
    assert not bad, bad[:5]
    for route in ("replay_lds_hist_fastdiv", "replay_lds_hist_ieee", "replay_lds_state_fastdiv", "replay_lds_state_ieee", "replay_hbm16_fastdiv",
                  "replay_hbm16_ieee"):
        assert stats.get(route, 0) >= 1, (route, stats)
    assert sum(stats.values()) >= 18, stats


def test_masked_module_sweep_equals_the_literal_batch_loop_also_in_the_coupled_class():
    n, reruns, reruns_large, bad = FP.run_module_masked(seed=21, N=40, verbose=False, large_every=5, grad_frac=0.4)
    print("run_module_masked:", {"cases": n, "coupled": reruns, "coupled_hybrid": reruns_large, "gradient_cases": FP.run_module_masked.ngrad})
    assert n >= 30 and not bad, bad[:5]
    # the sweep visits the coupled class, under autograd too, and on a hybrid-sized map (masked lock-step large-map kernel + batchloop_finish)
    assert reruns >= 4 and reruns_large >= 1 and FP.run_module_masked.ngrad >= 6, (reruns, reruns_large, FP.run_module_masked.ngrad)


@pytest.mark.parametrize("shape", RAY_SHAPES)
def test_each_filter_cell_searches_exactly_its_ray(shape):
    """one filter cell open: the search can only walk along its offset -- the path from the middle of the map to a goal k steps along it is
    exactly that ray, and nothing off the ray is ever closed"""
    H, W = shape
    rng = np.random.default_rng(H * 1000 + W)
    maps = np.ones((1, 1, H, W), np.float32)
    cost = rng.random((1, 1, H, W)).astype(np.float32)
    sr, sc = H // 2, W // 2
    k = min(H, W) // 2 - 1
    for bit in FP.SINGLE_BIT_MASKS:
        b = bit.bit_length() - 1
        dr, dc = FP.offset_of(b)
        ray = [(sr + i * dr) * W + (sc + i * dc) for i in range(k + 1)]
        start, goal = _onehot([ray[0]], H, W), _onehot([ray[-1]], H, W)
        hist, paths, iters, status, log = _search(cost, start, goal, maps, bit)
        assert int(status[0]) == 0, (shape, hex(bit))
        want = np.zeros(H * W, np.int64)
        want[ray] = 1
        assert np.array_equal(paths[0].cpu().numpy().reshape(-1), want), (shape, hex(bit))
        assert set(np.flatnonzero(hist[0].cpu().numpy())) <= set(ray), (shape, hex(bit))
        assert log[0, :k + 1].cpu().tolist() == ray and int(iters[0]) == k + 1, (shape, hex(bit))


@pytest.mark.parametrize("shape", RAY_SHAPES)
def test_moore8_minus_one_cell_detours_like_the_oracle(shape):
    """Moore-8 without one cell, the goal one step away along exactly the missing move: the search has to go round, as the oracle does"""
    H, W = shape
    rng = np.random.default_rng(7 * H + W)
    sr, sc = H // 2, W // 2
    maps = np.ones((1, 1, H, W), np.float32)
    for mask in FP.MOORE_MINUS_ONE_MASKS:
        b = (mask ^ FP.MOORE8).bit_length() - 1
        dr, dc = FP.offset_of(b)
        cost = (rng.random((1, 1, H, W)) * 10.0).astype(np.float32)
        start, goal = _onehot([sr * W + sc], H, W), _onehot([(sr + dr) * W + sc + dc], H, W)
        out = _search(cost, start, goal, maps, mask)
        o = O.forward(cost, start, goal, maps, 0.5, W * W, mode="sm", want_log=True, neighbor_mask=mask)
        assert FP.compare_masked_search(out, o, True), (shape, hex(mask))
        assert int(out[1].sum()) >= 3  # not the direct step


@pytest.mark.parametrize("mask", [0x1EE, 0x0E4])  # Moore-8 without filter cell (0,0); the directed set (+1,-1), (0,-1), (-1,+1), (-1,0)
@pytest.mark.parametrize("shape", [(260, 270), (512, 512)])
def test_masked_maps_above_65519_cells(shape, mask):
    """the long hybrid search and the replay with 32-bit history stamps under a filter that sets cells (0,2), (2,0), (2,2): forward against
    the state machine, dL/dcost against the dense reverse mode (short searches: the oracle scans every cell per step)"""
    from neural_astar.planner.differentiable_astar import DifferentiableAstar
    H, W = shape
    assert H * W > 65519 and FP.replay_route(H, W, W * W).startswith("replay_hbm32")
    rng = np.random.default_rng(H + mask)
    maps, st, gl = FP.masked_problems(rng, 2, H, W, mask, p=0.1, max_dist=6)
    cost = rng.random((2, 1, H, W)).astype(np.float32)
    o = O.forward(cost, st, gl, maps, 0.5, W * W, mode="sm", neighbor_mask=mask)
    assert o.status == 0
    da = DifferentiableAstar(0.5, 1.0).to(_dev()).eval()
    with torch.no_grad():
        da.neighbor_filter.copy_(torch.tensor(FP.mask_filter(mask), dtype=torch.float32).reshape(1, 1, 3, 3))
    c = _t(cost).requires_grad_(True)
    out = da(c, _t(st), _t(gl), _t(maps))
    assert np.array_equal(out.histories[:, 0].detach().cpu().numpy(), o.histories)
    assert np.array_equal(out.paths[:, 0].cpu().numpy(), o.paths)
    up = rng.standard_normal((2, 1, H, W)).astype(np.float32)
    (out.histories * _t(up)).sum().backward()
    ref = O.backward(up, cost, st, gl, maps, 0.5, W * W, neighbor_mask=mask)
    err = float(np.abs(c.grad[:, 0].cpu().numpy() - ref).max())
    assert err <= 1e-5 * max(1.0, float(np.abs(ref).max())), err


@pytest.mark.parametrize("shape", [(16, 16), (32, 32), (64, 64), (20, 24), (20, 45), (33, 31)])
def test_masked_placement_packed_output_and_ordered_replay(shape):
    """nastar_forward_ex_masked with a checked placement, order_out and packed_out equals the unplaced launch; its packed masks are the
    outputs packed; the masked replay in a placement order equals the one in the natural order"""
    from neural_astar import _native, ops, parallel
    H, W = shape
    B = 12
    dev = _dev()
    lib = _native.load()
    rng = np.random.default_rng(H * W)
    mask = 0x0E4 if W % 2 else 0x1AB
    maps, st, gl = FP.masked_problems(rng, B, H, W, mask, p=0.15)
    cost = rng.random((B, 1, H, W)).astype(np.float32)
    c, s, g, m = (_t(x[:, 0]) for x in (cost, st, gl, maps))
    T = W * W
    ref = ops.search_nograd(c, s, g, m, 0.5, T, want_log=True, neighbor_mask=mask)
    order = torch.from_numpy(rng.permutation(B).astype(np.int32)).to(dev)
    order_out = ops.new_placement_buffer(B, dev)
    hist = torch.empty((B, H, W), device=dev)
    paths = torch.empty((B, H, W), dtype=torch.int64, device=dev)
    iters = torch.empty((B,), dtype=torch.int32, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    log = torch.empty((B, T), dtype=torch.int32, device=dev)
    nb = (H * W + 7) // 8
    packed = torch.zeros((B, 2 * nb), dtype=torch.uint8, device=dev)
    ws = torch.zeros((16,), dtype=torch.uint8, device=dev)
    rc = lib.nastar_forward_ex_masked(c.data_ptr(), s.data_ptr(), g.data_ptr(), m.data_ptr(), B, H, W, 0.5, T, hist.data_ptr(), paths.data_ptr(),
                                      log.data_ptr(), iters.data_ptr(), status.data_ptr(), packed.data_ptr(), ws.data_ptr(), 16,
                                      ops.FORWARD_FLAGS | ops.FLAG_CHECK_ORDER, order.data_ptr(), order_out.data_ptr(), None, None, mask,
                                      torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    for x, y in zip((hist, paths, iters, status), ref[:4]):
        assert torch.equal(x, y), shape
    it = iters.cpu().numpy()
    for b in range(B):
        assert np.array_equal(log[b, :it[b]].cpu().numpy(), ref[4][b, :it[b]].cpu().numpy())
    assert sorted(order_out[:B].cpu().tolist()) == list(range(B)) and int(order_out[B]) == 0
    assert torch.equal(packed, parallel.pack_masks(hist.unsqueeze(1), paths.unsqueeze(1))), shape
    # the masked replay (nastar_backward_replay_ordered_masked) in the forward's completion order and in the natural order
    up = _t(rng.standard_normal((B, H, W)).astype(np.float32))
    t_batch = (iters.amax() - 1).to(torch.int32).reshape(1)
    g_nat = ops.astar_backward_replay(up, c, s, g, m, log, 0.5, T, iters, t_batch, None, 0, mask)
    g_ord = ops.astar_backward_replay(up, c, s, g, m, log, 0.5, T, iters, t_batch, order_out[:B].clone(), 0, mask)
    torch.cuda.synchronize()
    assert torch.equal(g_nat, g_ord), shape
    want = O.backward(up.cpu().numpy(), cost, st, gl, maps, 0.5, T, neighbor_mask=mask)
    assert float(np.abs(g_nat.cpu().numpy() - want).max()) <= 1e-5 * max(1.0, float(np.abs(want).max()))
