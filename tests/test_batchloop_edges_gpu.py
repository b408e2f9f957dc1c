"""GPU (-m gpu): the exact batch loop (nastar_forward_batchloop_finish and its masked / heuristic twins: PROBE, nastar_batchloop_tend_kernel,
FINAL) on the cases of tests/batchloop_edges.py, bit for bit against the CPU oracle's literal batch loop: batches of 1025 to 4096 maps (the
tend kernel's stride of 1024 over maps and over marked maps), the bit and word seams of the probe bitmap, budgets that end the loop, budgets
of half a million steps (the tend kernel's largest LDS launch, the first budget that ANDs in global memory, 600000 steps), maps that take no
part inside a large batch, and the placed autograd lane of DifferentiableAstar.forward() with its replay backward.  What each case reaches is
shown on the CPU by tests/test_batchloop_edges.py.  Every test prints its wall time on the device."""
import time
import warnings

import numpy as np
import pytest
import torch

import batchloop_edges as E

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _search(c, x, exact):
    """ops.search_nograd on the case's batch -> (hist, paths, iters, status, log or None) as numpy, seconds"""
    from neural_astar import ops
    kw = {}
    if c.mask is not None:
        kw["neighbor_mask"] = c.mask
    if c.zero_h:
        kw["heuristic"] = _t(x.h0)
    args = [_t(a) for a in x[:4]]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = ops.search_nograd(*args, c.g_ratio, c.budget, want_log=c.want_log, exact=exact, **kw)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    hist, paths, iters, status, log = (o.cpu().numpy() if o is not None else None for o in out[:5])
    return (hist, paths, iters, status, log if c.want_log else None), dt


def _rows_differ(a, b):
    return np.flatnonzero((a != b).reshape(a.shape[0], -1).any(1))


def _log_rows_differ(log, want, iters):
    """rows whose first iters[b] selections are not `want`'s"""
    live = np.arange(log.shape[1])[None, :] < iters[:, None]
    return np.flatnonzero(((log != want) & live).any(1))


def _check_plain(c, e, out):
    """the early-exit launch alone equals every map searched alone: what fails here is not the finish call's"""
    hist, paths, iters, status, log = out
    known = e.sm_status >= 0
    assert np.array_equal(status[known], e.sm_status[known]), f"{c.name} plain: status"
    assert _rows_differ(hist[known].view(np.uint32), e.sm_hist[known].view(np.uint32)).size == 0, f"{c.name} plain: histories"
    ok = e.ok
    assert np.array_equal(iters[ok], e.sm_iters[ok]), f"{c.name} plain: iters"
    assert _rows_differ(paths[ok], e.sm_paths[ok]).size == 0, f"{c.name} plain: paths"
    if c.want_log:
        assert _log_rows_differ(log[ok], e.sm_log[ok], iters[ok]).size == 0, f"{c.name} plain: selection log"


def _check_exact(c, e, out, plain):
    hist, paths, iters, status, log = out
    ok, T = e.ok, e.t_end + 1
    assert (status[ok] == 0).all(), f"{c.name}: status of maps {np.flatnonzero(ok & (status != 0))[:8]}"
    bad = _rows_differ(hist[ok].view(np.uint32), e.hist[ok].view(np.uint32))
    assert bad.size == 0, f"{c.name}: histories of {bad.size} maps differ from the batch loop's, first {np.flatnonzero(ok)[bad[:8]]} (t_end {e.t_end}, tmax {e.tmax})"
    bad = _rows_differ(paths[ok], e.paths[ok])
    assert bad.size == 0, f"{c.name}: paths of maps {np.flatnonzero(ok)[bad[:8]]}"
    d = e.differs
    assert (iters[d] == T).all(), f"{c.name}: a re-run map reports {iters[d][iters[d] != T][:8]} steps, the batch ran {T}"
    rest = ok & ~d
    assert ((iters[rest] == e.sm_iters[rest]) | (iters[rest] == T)).all(), f"{c.name}: iters of maps {np.flatnonzero(rest & (iters != e.sm_iters) & (iters != T))[:8]}"
    if d.any():
        assert int(iters[ok].max()) - 1 == e.t_end, f"{c.name}: the batch ended at step {int(iters[ok].max()) - 1}, the oracle's at {e.t_end}"
    if c.want_log:
        bad = _log_rows_differ(log[ok], e.log[ok], iters[ok])
        assert bad.size == 0, f"{c.name}: selection logs of maps {np.flatnonzero(ok)[bad[:8]]}"
    # a map that takes no part: what the plain launch returns for it
    for b in np.flatnonzero(~ok):
        assert status[b] == plain[3][b] != 0 and iters[b] == plain[2][b], f"{c.name}: failed map {b}"
        assert np.array_equal(hist[b].view(np.uint32), plain[0][b].view(np.uint32)) and np.array_equal(paths[b], plain[1][b]), f"{c.name}: failed map {b}"


def _run_case(name):
    c = E.table()[name]
    x, e = E.inputs(c), E.expected(c)
    plain, t_plain = _search(c, x, exact=False)
    _check_plain(c, e, plain)
    out, t_exact = _search(c, x, exact=True)
    print(f"{name}: B {len(c.maps)} {c.shape} budget {c.budget} tmax {e.tmax} t_end {e.t_end} differ {int(e.differs.sum())}: "
          f"plain {t_plain * 1e3:.1f} ms, exact {t_exact * 1e3:.1f} ms")
    _check_exact(c, e, out, plain)
    return c, e, out


@pytest.mark.parametrize("name", E.names("A"))
def test_large_batches(name):
    _run_case(name)


@pytest.mark.parametrize("name", E.names("B"))
def test_bit_and_word_seams(name):
    _run_case(name)


@pytest.mark.parametrize("name", E.names("C"))
def test_budgets_that_end_the_loop(name):
    c, e, out = _run_case(name)
    assert (out[2] == c.max_iters).all()  # every map of these batches is re-run or budget-ended


@pytest.mark.parametrize("name", E.names("D"))
def test_long_budgets(name):
    """the PROBE runs the marked maps for the whole budget; the tend kernel ANDs `nw` words per marked map -- in LDS up to
    batchloop_edges.TEND_LDS_WORDS, in global memory above.  A launch that the runtime refuses surfaces as the call's error."""
    _run_case(name)


@pytest.mark.parametrize("name", E.names("E"))
def test_maps_that_take_no_part(name):
    c, e, out = _run_case(name)
    assert (out[3][list(c.walled + c.no_start)] == E.STATUS_UNSOLVABLE).all()


@pytest.mark.parametrize("name", E.names("F"))
def test_masked_and_heuristic_finish_calls(name):
    _run_case(name)


# ---- the module ------------------------------------------------------------------------------------------------------------------------------
def _maps4(x):
    return tuple(_t(a[:, None]) for a in x[:4])


@pytest.mark.parametrize("name,train,Tmax", [("A_16x16_4096", False, 1.0), ("C_budget_64", True, 0.25)])
def test_module_without_gradients_in_every_checking_mode(name, train, Tmax):
    import neural_astar.planner.differentiable_astar as DA
    c = E.table()[name]
    e = E.expected(c)
    cost, start, goal, passable = _maps4(E.inputs(c))
    t0 = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for mode in (True, "deferred", False):
            da = DA.DifferentiableAstar(c.g_ratio, Tmax, check_solvable=mode).to(cost.device).train(train)
            assert DA.ops.max_iters_for(c.shape[1], da.Tmax, da.training) == c.budget
            with torch.no_grad():
                out = da(cost, start, goal, passable)
                da.raise_if_unsolvable()
            assert np.array_equal(out.histories[:, 0].cpu().numpy(), e.hist), (name, mode)
            assert np.array_equal(out.paths[:, 0].cpu().numpy(), e.paths), (name, mode)
    print(f"{name}: three module calls {time.perf_counter() - t0:.2f} s")


GRAD_CASES = ["A_16x16_1025", "A_16x16_2100", "A_8x8_1025", "A_8x8_2100"]


@pytest.mark.parametrize("name", GRAD_CASES)
def test_placed_autograd_lane_runs_the_exact_pipeline_and_its_replay(name, monkeypatch):
    """B >= ops.PLACEMENT_MIN_BATCH under autograd: forward() takes ops.astar_forward_placed(exact=True); the replay backward is ordered by
    the early-exit launch's completion order while its iters / t_batch are the FINAL launch's.  Gradient bar: 1e-5 * max(1, max|ref|), the
    one of tests/test_coupled_forward.py."""
    import neural_astar.planner.differentiable_astar as DA
    from oracle import oracle as O
    c = E.table()[name]
    e = E.expected(c)
    x = E.inputs(c)
    B = len(c.maps)
    assert B >= DA.ops.PLACEMENT_MIN_BATCH and e.differs.any()
    calls = []
    placed = DA.ops.astar_forward_placed
    monkeypatch.setattr(DA.ops, "astar_forward_placed", lambda *a, **k: (calls.append(k.get("exact")), placed(*a, **k))[1])
    cost, start, goal, passable = _maps4(x)
    up = np.random.Generator(np.random.PCG64(B)).standard_normal((B, 1) + c.shape).astype(np.float32)
    ref = O.backward(up, *x[:4], c.g_ratio, c.budget)
    t0 = time.perf_counter()
    da = DA.DifferentiableAstar(c.g_ratio, 1.0).to(cost.device).eval()
    cost.requires_grad_()
    out = da(cost, start, goal, passable)
    (out.histories * _t(up)).sum().backward()
    grad = cost.grad[:, 0].cpu().numpy()
    dt = time.perf_counter() - t0
    assert calls == [True], calls
    assert np.array_equal(out.histories[:, 0].detach().cpu().numpy(), e.hist)
    err, scale = float(np.abs(grad - ref).max()), max(1.0, float(np.abs(ref).max()))
    print(f"{name}: forward + backward {dt * 1e3:.1f} ms, worst gradient error {err:.3e} (max|ref| {float(np.abs(ref).max()):.3e}, bar {1e-5 * scale:.3e})")
    assert err <= 1e-5 * scale, err


def test_fused_l1_step_on_a_large_coupled_batch():
    """utils.training.fused_l1_step (L1 loss + sign gradient inside the replay) at B = 1025 against the oracle's reverse mode of the L1 sign gradient"""
    import torch.nn as nn
    from neural_astar.planner import VanillaAstar
    from neural_astar.utils.training import fused_l1_step
    from oracle import oracle as O
    c = E.table()["A_16x16_1025"]
    e = E.expected(c)
    x = E.inputs(c)
    cost, start, goal, passable = _maps4(x)
    va = VanillaAstar(g_ratio=c.g_ratio).to(cost.device).eval()
    opt = e.paths[:, None].astype(np.float32)

    class _P(nn.Module):  # a planner whose cost map is a leaf (fused_l1_step's NeuralAstar surface)
        learn_obstacles = False
        use_differentiable_astar = True

        def __init__(self):
            super().__init__()
            self.astar = va.astar
            self.cost = nn.Parameter(cost.clone())

        def encode(self, m, st, gl):
            return self.cost
    pl = _P()
    t0 = time.perf_counter()
    loss, out = fused_l1_step(pl, passable, start, goal, _t(opt))
    loss.backward()
    grad = pl.cost.grad[:, 0].cpu().numpy()
    dt = time.perf_counter() - t0
    assert np.array_equal(out.histories[:, 0].cpu().numpy(), e.hist)
    hist4 = e.hist[:, None]
    up = (np.sign(hist4 - opt) / hist4.size).astype(np.float32)
    ref = O.backward(up, *x[:4], c.g_ratio, c.budget)
    assert abs(float(loss.detach()) - float(np.abs(hist4 - opt).mean())) < 1e-6
    err, scale = float(np.abs(grad - ref).max()), max(1.0, float(np.abs(ref).max()))
    print(f"fused_l1_step at B 1025: {dt * 1e3:.1f} ms, worst gradient error {err:.3e} (max|ref| {float(np.abs(ref).max()):.3e})")
    assert err <= 1e-5 * scale, err


def test_exact_outputs_are_a_pure_function_of_the_batch():
    """the same batch twice, and once reversed: the same bits, permuted (the tend kernel's atomics and the stride over maps leave no trace of
    the order in which maps or threads arrive)"""
    c = E.table()["A_16x16_2100"]
    x = E.inputs(c)
    t0 = time.perf_counter()
    first, _ = _search(c, x, exact=True)
    again, _ = _search(c, x, exact=True)
    flipped, _ = _search(c, E.Inputs(*(np.ascontiguousarray(a[::-1]) for a in x[:4]), None), exact=True)
    print(f"three exact runs of {c.name}: {time.perf_counter() - t0:.2f} s")
    live = np.arange(first[4].shape[1])[None, :] < first[2][:, None]
    for k, (a, b, f) in enumerate(zip(first, again, flipped)):
        if k == 4:
            a, b, f = (np.where(live, v, -1) for v in (a, b, f[::-1]))  # (log entries past iters[b] are never written)
            assert np.array_equal(a, b) and np.array_equal(a, f)
        else:
            assert np.array_equal(a, b) and np.array_equal(a, f[::-1]), k
