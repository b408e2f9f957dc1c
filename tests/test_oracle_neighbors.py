"""CPU: the oracle's neighbourhood gate (oracle/nastar_oracle.c, the *_masked entry points) pinned by the reference's vectors with a
non-default neighbor_filter (tests/golden/neighbors/), by torch's own conv2d for the orientation of every filter cell, and by the agreement of
its two restatements (dense tensor program, state machine) under all 256 masks.  The masked GPU sweeps (tools/fuzz_parity.py run_masked /
run_backward_masked / run_module_masked) rest on this."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import golden_util as G
import neighbor_golden as NG
from oracle import oracle as O

MOORE8 = 0x1EF
MASKS_CENTRE_CLEAR = [m for m in range(512) if not m & 0x10]


def _onehot(idx, B, H, W):
    return np.eye(H * W, dtype=np.float32)[np.asarray(idx)].reshape(B, 1, H, W)


@pytest.mark.parametrize("mode", ["dense", "sm"])
@pytest.mark.parametrize("name", NG.names())
def test_masked_oracle_reproduces_the_reference_with_its_filter(name, mode):
    g = NG.load(name)
    m = NG.mask_of(g.filter)
    o = O.forward(g.cost_maps, g.start_maps, g.goal_maps, g.map_designs, g.g_ratio, g.max_iters, mode=mode, want_log=True, neighbor_mask=m)
    assert o.status == 0
    assert np.array_equal(o.histories, g.histories[:, 0]), f"{name} ({mode}): histories"
    assert np.array_equal(o.paths, g.paths[:, 0]), f"{name} ({mode}): paths"
    assert o.t_batch == g.t_batch
    T = g.sel_log.shape[1]
    if mode == "dense":  # the literal batch loop: every loop step of every map, the goal re-selected after it was reached
        assert np.array_equal(o.sel_log[:, :T], g.sel_log)
        assert (o.sel_log[:, T:] == -1).all()
    else:  # per-map early exit: the selections up to and including the goal
        for b in range(g.sel_log.shape[0]):
            n = int(o.iters[b])
            assert np.array_equal(o.sel_log[b, :n], g.sel_log[b, :n]), f"{name}: map {b}"
            assert n == T or o.sel_log[b, n - 1] == g.goal_maps[b].argmax()
    if g.inter_hist is not None:
        # the reference's intermediate_results: loop step t stores the histories before its update and the one-hot of its selection; then
        # one final entry (the outputs)
        B, _, H, W = g.map_designs.shape
        assert g.inter_hist.shape[0] == T + 1
        hist = np.zeros((B, H * W), np.float32)
        for t in range(T):
            assert np.array_equal(hist.reshape(B, 1, H, W), g.inter_hist[t]), t
            step = g.inter_path[t].reshape(B, -1)
            assert (step.sum(1) == 1).all() and np.array_equal(step.argmax(1), o.sel_log[:, t]), t
            hist[np.arange(B), o.sel_log[:, t]] = 1.0
        assert np.array_equal(g.inter_hist[T][:, 0], o.histories) and np.array_equal(g.inter_path[T][:, 0], o.paths.astype(np.float32))


@pytest.mark.parametrize("name", [n for n in NG.names() if n.startswith("grad_")])
def test_masked_oracle_backward_matches_the_reference_l1_gradient(name):
    g = NG.load(name)
    h = torch.from_numpy(g.histories).requires_grad_(True)
    (up,) = torch.autograd.grad(torch.nn.L1Loss()(h, torch.from_numpy(g.target)), h)  # dL/dhistories of the reference's loss
    got = O.backward(up.numpy(), g.cost_maps, g.start_maps, g.goal_maps, g.map_designs, g.g_ratio, g.max_iters,
                     neighbor_mask=NG.mask_of(g.filter))
    ref = g.grad_cost[:, 0]
    assert float(np.abs(got - ref).max()) <= 1e-5 * max(1.0, float(np.abs(ref).max()))
    # ... and the filter matters: the Moore-8 oracle computes another gradient on the same inputs
    moore = O.backward(up.numpy(), g.cost_maps, g.start_maps, g.goal_maps, g.map_designs, g.g_ratio, g.max_iters)
    assert float(np.abs(moore - ref).max()) > 1e-2 * float(np.abs(ref).max())


@pytest.mark.parametrize("name", G.names())
def test_moore8_mask_equals_the_entry_points_without_a_mask(name):
    g = G.load(name)
    log = g.sel_log is not None
    for mode in ("dense", "sm"):
        a = O.forward(g.cost_maps, g.start_maps, g.goal_maps, g.passable, g.g_ratio, g.max_iters, mode=mode, want_log=log, neighbor_mask=None)
        b = O.forward(g.cost_maps, g.start_maps, g.goal_maps, g.passable, g.g_ratio, g.max_iters, mode=mode, want_log=log, neighbor_mask=MOORE8)
        assert a.status == b.status and a.t_batch == b.t_batch
        for x, y in ((a.histories, b.histories), (a.paths, b.paths), (a.iters, b.iters), (a.sel_log, b.sel_log)):
            assert (x is None and y is None) or np.array_equal(x, y), mode
    if name.startswith("grad_"):
        args = (g.grad_up, g.cost_maps, g.start_maps, g.goal_maps, g.passable, g.g_ratio, g.max_iters)
        assert np.array_equal(O.backward(*args, neighbor_mask=None), O.backward(*args, neighbor_mask=MOORE8))


@pytest.mark.parametrize("bit", [0, 1, 2, 3, 5, 6, 7, 8])
def test_each_filter_cell_opens_the_offset_conv2d_marks(bit):
    """one filter cell on an open 7x7 map, the start in the middle: the second selection is the one cell F.conv2d(one_hot(start), filter,
    padding=1) marks -- the orientation pinned by torch's definition, not by the oracle's own reading of it"""
    H = W = 7
    start = _onehot([3 * W + 3], 1, H, W)
    goal = _onehot([0], 1, H, W)
    maps = np.ones((1, 1, H, W), np.float32)
    filt = torch.zeros(1, 1, 3, 3)
    filt.view(-1)[bit] = 1.0
    marked = F.conv2d(torch.from_numpy(start), filt, padding=1).reshape(-1).numpy()
    assert (marked != 0).sum() == 1
    o = O.forward(maps, start, goal, maps, 0.5, 2, mode="sm", want_log=True, neighbor_mask=1 << bit)
    assert o.sel_log[0, 0] == 3 * W + 3 and o.sel_log[0, 1] == int(np.flatnonzero(marked)[0])
    d = O.forward(maps, start, goal, maps, 0.5, 2, mode="dense", want_log=True, neighbor_mask=1 << bit)
    assert np.array_equal(d.sel_log, o.sel_log)


def test_masks_outside_the_encoding_are_refused():
    maps = np.ones((1, 1, 4, 4), np.float32)
    for bad in (0x10, 0x1FF, 0x200, -1):
        with pytest.raises(ValueError):
            O.forward(maps, _onehot([0], 1, 4, 4), _onehot([15], 1, 4, 4), maps, neighbor_mask=bad)


def _reachable(passable, s, mask):
    """cells the search opens from s under mask: a plain flood over the offsets conv2d opens (filter cell (a, b) -> offset (1 - a, 1 - b))"""
    H, W = passable.shape
    moves = [(1 - k // 3, 1 - k % 3) for k in range(9) if mask >> k & 1]
    seen = np.zeros(H * W, bool)
    seen[s] = True
    stack = [s]
    while stack:
        r, c = divmod(stack.pop(), W)
        for dr, dc in moves:
            rr, cc = r + dr, c + dc
            if 0 <= rr < H and 0 <= cc < W and passable[rr, cc] and not seen[rr * W + cc]:
                seen[rr * W + cc] = True
                stack.append(rr * W + cc)
    return seen


def test_dense_equals_the_state_machine_for_every_mask():
    """the fixed point behind the per-map early exit does not depend on the move set -- the heuristic is >= 1 at every
    neighbour of the goal --, so with costs >= 0 and g_ratio in [0.5, 1) the literal batch loop and the state machine agree under any filter"""
    rng = np.random.default_rng(2026)
    solved = 0
    for mask in MASKS_CENTRE_CLEAR:
        for _ in range(2):
            B, H, W = int(rng.integers(1, 5)), int(rng.integers(2, 10)), int(rng.integers(2, 12))
            maps = (rng.random((B, H, W)) > 0.2).astype(np.float32)
            sidx, gidx = np.zeros(B, np.int64), np.zeros(B, np.int64)
            for b in range(B):
                sidx[b] = rng.integers(H * W)
                reach = _reachable(maps[b], int(sidx[b]), mask)
                reach[sidx[b]] = False
                cand = np.flatnonzero(reach)
                gidx[b] = cand[rng.integers(cand.size)] if cand.size else sidx[b]
                solved += cand.size > 0
            cost = (rng.random((B, H, W)) * rng.choice([1.0, 10.0]) * (rng.random((B, H, W)) < 0.7)).astype(np.float32)
            gr = float(rng.uniform(0.5, 1.0))
            args = (cost, _onehot(sidx, B, H, W), _onehot(gidx, B, H, W), maps, gr, W * W)
            a = O.forward(*args, mode="dense", want_log=True, neighbor_mask=mask)
            b = O.forward(*args, mode="sm", want_log=True, neighbor_mask=mask)
            assert a.status == 0 and b.status == 0, hex(mask)
            assert np.array_equal(a.histories, b.histories) and np.array_equal(a.paths, b.paths), hex(mask)
            assert np.array_equal(a.iters, b.iters), hex(mask)
            for i in range(B):
                n = int(b.iters[i])
                assert np.array_equal(a.sel_log[i, :n], b.sel_log[i, :n]), hex(mask)
    assert solved >= 600  # most problems do search (a goal apart from the start)


def test_reference_vectors_separate_the_filter_cells_moore8_shares():
    """the reference vectors tell the filter cells (0,2), (2,0), (2,2) apart: each is set by a vector that is not Moore-8, and (0,2) / (2,0),
    which von Neumann, diagonals-only and Moore-8 treat alike, each appear without the other"""
    masks = {NG.mask_of(NG.load(n).filter) for n in NG.names()} - {MOORE8}
    for bit in (2, 6, 8):
        assert any(m >> bit & 1 for m in masks), bit
    assert any(m & 0x004 and not m & 0x040 for m in masks) and any(m & 0x040 and not m & 0x004 for m in masks)
    assert any(NG.load(n).g_ratio == 0.8 and float(NG.load(n).cost_maps.max()) > 1.0 for n in NG.names())
