"""CPU half of the replay backward's edge tests (tests/replay_edges.py holds the problems; tests/test_replay_edges_gpu.py runs the kernels).
The oracle ALONE must meet every condition the GPU tests rely on -- no unsolvable map, a finite gradient that is exactly 0.0 outside the
opened cells, short maps whose whole gradient is the batch coupling, budgets that end at and one step before the far goal -- and the
shapes must reach every replay route of csrc/nastar_capi.hip backward_replay_impl.  The last tests perturb the EXPECTATION the way a wrong
kernel would (no `extra` copies, one cell off by 1e-4 of the map's scale, a stray write, an unwritten cell) and see the shared checker
refuse each one."""
import concurrent.futures
import itertools
import os

import numpy as np
import pytest

import replay_edges as R

CASES = list(itertools.product(R.SHAPES, R.VARIANTS))
# the budget W * W of a one-column map is ONE step and a 1x1 map has one cell: the far search ends in its first step whatever the variant
ONE_STEP = ("40x1", "1x1")


@pytest.fixture(scope="module", autouse=True)
def _oracle_answers():
    """every case's oracle run, several at a time (the calls release the GIL; g_ratio 1 on the largest maps is a 700-step dense run)"""
    R.case("1x1", "u01")  # (loads the oracle library once, before the threads)
    with concurrent.futures.ThreadPoolExecutor(max(1, min(8, (os.cpu_count() or 2) // 2))) as pool:
        list(pool.map(lambda sv: R.case(sv[0], "u01") and R.case(*sv), CASES))


def test_shapes_reach_every_replay_route_and_both_hand_scheduled_sizes():
    from fuzz_parity import replay_route
    table = {s: R.route(s, R.SHAPES[s][1] ** 2) for s in R.SHAPES}
    for s, r in table.items():
        print(f"{s:>10}  {r}")
        assert r == R.SHAPES[s][4], (s, r)
    names = {f"replay_{kind}_{div}" for kind in ("lds_hist", "lds_state", "hbm16", "hbm32") for div in ("fastdiv", "ieee")}
    # every name replay_route can return: probe it over sizes on both sides of each of its thresholds
    probed = {replay_route(H, W, T) for H, W in ((8, 8), (9, 7), (64, 64), (60, 66), (120, 120), (112, 128), (256, 257), (257, 256))
              for T in (1, W * W, 70000)}
    assert probed == names
    assert set(table.values()) == names | {"asm"}
    assert {(R.SHAPES[s][0], R.SHAPES[s][1]) for s, r in table.items() if r == "asm"} == {(32, 32), (16, 16)}
    # the view 4 bytes past a 16-byte boundary fails the hand-scheduled loop's alignment test: the compiled loop at the same size
    assert R.SHAPES["32x32+4B"][:2] == (32, 32) and table["32x32+4B"] == "replay_lds_hist_fastdiv"
    # a short budget moves the step history into LDS; the hand-scheduled loop and the HBM state stay
    assert R.route("64x64", 3) == "replay_lds_hist_fastdiv" and R.route("32x32", 1) == "asm" and R.route("110x110", 1) == "replay_hbm16_ieee"


@pytest.mark.parametrize("shape,variant", CASES)
def test_oracle_meets_the_conditions_the_gpu_tests_rely_on(shape, variant):
    c = R.case(shape, variant)
    assert c.fwd.status == 0 and not c.fwd.map_status.any(), "an unsolvable map"
    assert np.isfinite(c.ref).all()
    assert not c.ref[~c.opened].any(), "the oracle's gradient is not exactly 0.0 outside the opened cells"
    assert c.opened.reshape(3, -1).sum(1).min() >= 1 and (c.opened <= (c.m[:, 0] > 0) | (c.s[:, 0] > 0)).all()
    if variant in R.EXACTLY_ZERO:
        assert not c.ref.any()
    assert c.fwd.iters[0] == 1 and 1 <= c.fwd.iters.max() <= c.T


@pytest.mark.parametrize("shape", list(R.SHAPES))
def test_the_short_maps_gradient_is_all_batch_coupling(shape):
    """map 0 (start == goal) waits t_batch steps at its fixed point: in the coupled batch its gradient is those `extra` copies and nothing
    else -- as a batch of its own it is exactly zero.  A replay that dropped or miscounted the copies is wrong by ALL of this gradient."""
    c = R.case(shape, "u01")
    solo = R.alone(c)
    assert not solo[0].any()
    if c.fwd.iters[2] > 1:
        assert np.abs(c.ref[0]).max() > 0.05, "the coupled gradient of the start == goal map"
        assert np.abs(c.ref[1] - solo[1]).max() > 0.05 or c.fwd.iters[1] == c.fwd.iters[2]
    else:
        assert shape in ONE_STEP and not c.ref.any()


@pytest.mark.parametrize("shape", list(R.SHAPES))
def test_budgets_end_at_and_one_step_before_the_far_goal(shape):
    at, before = R.case(shape, "Tgoal"), R.case(shape, "Tgoal-1")
    goal = at.g[2, 0] > 0
    if shape == "40x1":  # (one step of budget: the far goal is 39 cells away)
        assert at.T == before.T == 1 and at.fwd.histories[2][goal] == 0
        return
    assert at.T == at.fwd.iters[2] == R.case(shape, "u01").fwd.iters[2] and at.fwd.sel_log[2, at.T - 1] == np.flatnonzero(goal.reshape(-1))[0]
    assert at.fwd.histories[2][goal] == 1, "T = iters[2]: the far goal is selected on the last step of the budget"
    if shape == "1x1":   # (no budget below one step)
        assert before.T == 1
        return
    assert before.T == at.T - 1 and before.fwd.iters[2] == before.T
    assert before.fwd.histories[2][goal] == 0, "T = iters[2] - 1: the budget ends before the far goal is selected"


# ---- the shared checker refuses what a wrong kernel would produce --------------------------------------------------------------------------

COUPLED = [s for s in R.SHAPES if s not in ONE_STEP]


@pytest.mark.parametrize("shape", COUPLED)
def test_checker_refuses_a_gradient_without_the_extra_copies(shape):
    c = R.case(shape, "u01")
    R.check_grad(c.ref.copy(), c.ref, c.opened, c.route, "the oracle itself")
    with pytest.raises(AssertionError, match="map 0"):
        R.check_grad(R.alone(c), c.ref, c.opened, c.route, "no extra copies")


@pytest.mark.parametrize("shape", COUPLED)
def test_checker_refuses_one_cell_off_by_1e_4_of_the_maps_scale(shape):
    """(the per-batch form of the project's bar lets this pass on every map here: 1e-4 of a scale below 0.1 is under 1e-5)"""
    c = R.case(shape, "u01")
    for b in range(3):
        scale = np.abs(c.ref[b]).max()
        if scale < R.REL_FLOOR:
            assert shape == "1x40" and b == 2  # (the far map of the one-row batch: every step has ONE open cell, the gradient is zero)
            continue
        bad = c.ref.copy()
        r, col = np.argwhere(c.opened[b])[-1]
        bad[b, r, col] += np.float32(1e-4 * scale)
        with pytest.raises(AssertionError, match=f"map {b} "):
            R.check_grad(bad, c.ref, c.opened, c.route, "one cell shifted")


@pytest.mark.parametrize("shape", COUPLED)
def test_checker_refuses_a_stray_write_and_an_unwritten_cell(shape):
    c = R.case(shape, "u01")
    if (~c.opened).any():
        bad = c.ref.copy()
        b, r, col = np.argwhere(~c.opened)[-1]
        bad[b, r, col] = np.float32(1e-30)
        with pytest.raises(AssertionError, match="outside the opened cells"):
            R.check_grad(bad, c.ref, c.opened, c.route, "stray write")
    bad = c.ref.copy()
    bad[2, -1, -1] = np.nan
    with pytest.raises(AssertionError, match="NaN"):
        R.check_grad(bad, c.ref, c.opened, c.route, "unwritten cell")
