"""CPU tests of the large-map search's edge scenarios (tests/hybrid_edges.py) and of the emulator of its open-list bookkeeping
(tests/hybrid_emulator.py): no GPU.

  * every scenario meets its coverage conditions on the CPU oracle's own selection log -- the inputs do reach the seams they are aimed at;
  * the emulator without a defect reproduces the oracle's log, step count and status on every scenario, so it restates the same search;
  * each planted defect changes the log or the status of the scenarios named in CAUGHT_BY, and of none named in MISSED_BY: the table shows
    what every row is there for.  tests/test_hybrid_edges_gpu.py runs the same scenarios through the kernels.

``row_nocorr`` is caught by no scenario, and cannot be: below 2^22 cells the uncorrected quotient is already the row (the bound is in
``test_the_row_division_needs_no_correction_on_any_accepted_map``, which also checks it cell by cell on the extreme shapes).
"""
import functools

import numpy as np
import pytest

import hybrid_edges as E
import hybrid_emulator as EM

NAMES = list(E.table()) + [f"budget_{b}" for b in E.BUDGETS]
SEARCH_NAMES = [n for n in NAMES if not n.startswith("lock_")]
LOCK_NAMES = [n for n in NAMES if n.startswith("lock_")]
PAD_NAMES = [n for n in NAMES if n.startswith("pad_")]
THIN_NAMES = [n for n in NAMES if n.startswith("thin_")]

# defect -> the scenarios whose log or status it changes (lock_goal_closed: in lock-step mode, map 0 of the batch)
CAUGHT_BY = {
    "nbr_super": ["spl1_90x91_tie", "spl2_513x512_tie", "spl2_513x512_rnd", "spl2_512x514_tie", "spl3_700x1100_tie", "spl4_1024x1024_tie",
                  "spl5_1024x1152_tie", "wall_513x512", "budget_33"],
    "last_entry": ["spl2_513x512_tie", "spl2_512x514_tie", "spl3_700x1100_tie", "spl4_1024x1024_tie", "spl5_1024x1152_tie"],
    "own_lane": ["spl2_513x512_rnd", "spl2_512x514_rnd", "spl3_700x1100_rnd", "spl4_1024x1024_rnd", "spl5_1024x1152_rnd", "spl5_1024x1152_rnd_g0",
                 "thin_1x1179648_far", "thin_393216x3_far", "wall_513x512", "multihot_far", "budget_31"],
    "pad_open": PAD_NAMES,
    "row_nocorr": [],
    "lock_goal_closed": LOCK_NAMES,
}
# ... and some it cannot change: no ties without unit costs, one entry per lane at spl 1, no other super-chunk in a corridor, no padded cells
MISSED_BY = {
    "nbr_super": ["thin_1179648x1_far", "pad_81x81_tie"],
    "last_entry": ["spl1_90x91_tie", "spl5_1024x1152_rnd"],
    "own_lane": ["spl1_90x91_tie", "spl1_90x91_rnd", "thin_6400x1_far"],
    "pad_open": ["spl1_90x91_rnd", "thin_1x6400_far"],
    "row_nocorr": THIN_NAMES,
    "lock_goal_closed": [],
}


@functools.lru_cache(maxsize=None)
def oracle_run(name, mode="sm"):
    """(logs [B][iters], iters [B], status [B] or the batch's, t_batch) of the CPU oracle on scenario `name`; start / goal maps that are not
    one-hot go in as the one-hot of their highest cell"""
    from oracle import oracle as O
    sc = E.build(name, steps_of)
    o = O.forward(sc.cost, E.last_onehot(sc.start), E.last_onehot(sc.goal), sc.passable, sc.g_ratio, sc.max_iters, mode=mode, want_log=True)
    B = sc.cost.shape[0]
    n = [int(o.iters[b]) if mode == "sm" else o.t_batch + 1 for b in range(B)]
    status = [int(x) for x in o.map_status] if mode == "sm" else [int(o.status)] * B
    return [o.sel_log[b, :n[b]].copy() for b in range(B)], n, status, o.t_batch, o.histories.reshape(B, -1)


def steps_of(name):
    return oracle_run(name)[1][0]


@functools.lru_cache(maxsize=None)
def emulate(name, defect=None, lock=False):
    sc = E.build(name, steps_of)
    lock_steps = oracle_run(name, "dense")[3] + 1 if lock else None
    return [EM.run(sc.cost[b], sc.start[b], sc.goal[b], sc.passable[b], sc.g_ratio, sc.max_iters, defect=defect, lock_steps=lock_steps)
            for b in range(sc.cost.shape[0])]


def _same(a, b):
    return a[1] == b[1] and a[2] == b[2] and np.array_equal(a[0], b[0])


def test_the_table_holds_what_the_seams_need():
    """every spl from 1 to 5 with both division routes at spl 2, the thin shapes, the two padded shapes -- and every scenario a hybrid-sized map"""
    spls = {E.geometry(H, W)[3] for H, W in E.LADDER_SHAPES}
    assert spls == {1, 2, 3, 4, 5} and E.geometry(1024, 1152)[0] == 1179648
    assert all(H * W >= 6400 for H, W in E.LADDER_SHAPES + E.THIN_SHAPES + E.PAD_SHAPES)
    assert [H * W % 64 for H, W in E.PAD_SHAPES] == [33, 29] and 83 * 79 % 4 != 0
    for name in NAMES:
        sc = E.build(name, lambda n: 702)
        B, H, W = sc.cost.shape
        assert sc.name == name and all(a.shape == (B, H, W) and a.dtype == np.float32 for a in sc[1:5])
        s, g = np.flatnonzero(E.last_onehot(sc.start)[0]), np.flatnonzero(E.last_onehot(sc.goal)[0])
        rs, cs, rg, cg = *divmod(int(s[0]), W), *divmod(int(g[0]), W)
        assert (10 <= max(abs(rs - rg), abs(cs - cg)) <= 30) or name.startswith(("wall_", "lock_")), name


@pytest.mark.parametrize("name", SEARCH_NAMES)
def test_scenario_meets_its_conditions_and_the_emulator_equals_the_oracle(name):
    logs, iters, status, _, _ = oracle_run(name)
    sc = E.build(name, steps_of)
    _, H, W = sc.cost.shape
    cen = E.census(logs[0], iters[0], H, W)
    print(name, cen)
    row = E.table().get(name)
    if row is not None:
        assert E.unmet(row.cond, cen, status[0], H, W) == []
    else:  # a budget row: the search is cut off at exactly its budget, unsolved
        assert iters[0] == sc.max_iters and status[0] == 0 and int(logs[0][-1]) != int(np.flatnonzero(sc.goal)[0])
    assert _same(emulate(name)[0], (logs[0], iters[0], status[0]))


@pytest.mark.parametrize("name", LOCK_NAMES)
def test_lock_step_scenario_is_batch_coupled_beyond_the_first_super_chunk(name):
    """the literal batch loop closes more cells of map 0 than its own search does, all of them in super-chunk 1; map 1 is at a fixed point.
    The emulator equals the state machine, and in lock-step mode the batch loop's log of map 0."""
    logs, iters, status, _, hist = oracle_run(name)
    dlogs, dn, dstatus, t_batch, dhist = oracle_run(name, "dense")
    assert status == [0, 0] and dstatus == [0, 0] and t_batch + 1 >= max(iters)
    diff = np.flatnonzero(hist[0] != dhist[0])
    print(name, "cells the batch loop closes beyond the map's own search:", diff.size, "first", diff.min())
    assert diff.size > 0 and diff.min() >= E.table()[name].cond["min_coupled_cell"] and np.array_equal(hist[1], dhist[1])
    sc = E.build(name)
    assert 4096 <= int(np.flatnonzero(sc.goal[0])[0]) < 4160
    for b in range(2):
        assert _same(emulate(name)[b], (logs[b], iters[b], status[b]))
    assert np.array_equal(emulate(name, None, True)[0][0], dlogs[0])


@pytest.mark.parametrize("defect", EM.DEFECTS)
def test_planted_defect_is_caught_by_its_scenarios(defect):
    lock = defect == "lock_goal_closed"
    caught = [n for n in CAUGHT_BY[defect] if not _same(emulate(n, defect, lock)[0], emulate(n, None, lock)[0])]
    missed = [n for n in MISSED_BY[defect] if _same(emulate(n, defect, lock)[0], emulate(n, None, lock)[0])]
    assert caught == CAUGHT_BY[defect] and missed == MISSED_BY[defect]
    assert CAUGHT_BY[defect] or defect == "row_nocorr"
    if defect == "pad_open":  # the defective kernel selects a padded cell at once: the restatement stops where the kernel would leave the map
        assert all(emulate(n, defect)[0][2] == EM.FAULT for n in PAD_NAMES)


def test_the_row_division_needs_no_correction_on_any_accepted_map():
    """hybrid_row: r0 = (int)(fl(fl(i + 0.5) * fl(1 / W))).  i + 0.5 is exact below 2^23; the two roundings put the product within
    (r + 1) 2^-23 (1 + 2^-24) of (i + 0.5) / W, which lies at least 0.5 / W from an integer: r0 is the row whenever (r + 1) W <= H W < 2^22,
    that is, on every map the library takes (at most 1,179,648 cells).  The correction step is a margin that is never used -- checked here
    cell by cell on the thin shapes, on the largest map and on the widest row index times width, with the step taken out."""
    for H, W in E.THIN_SHAPES + [(1024, 1152), (1152, 1024), (3, 393216), (2, 589824), (1086, 1086), (700, 1100)]:
        assert H * W < 1 << 22
        m = EM._Map(np.zeros((1, 1), np.float32), np.ones((1, 1)), np.ones((1, 1)), np.ones((1, 1)), 0.5, "row_nocorr")
        m.H, m.W, m.inv_W = H, W, np.float32(1.0) / np.float32(W)
        i = np.arange(H * W, dtype=np.int64)
        r, c = m.row(i)
        assert np.array_equal(r, i // W) and np.array_equal(c, i % W), (H, W)
