"""GPU tests (-m gpu) of the guard rows in the LDS layout of the hand-scheduled search kernels and of the stored-heuristic step that relies
on them (csrc/nastar_search_compact.hip.h: carve_compact_asm_lds; csrc/nastar_search_asm5.hip.h).

The step no longer tests whether a neighbour lies inside the map: the COLUMNS come from a per-lane lookup of the selected cell's column, the
ROWS from the data -- a neighbour in "row -1" or "row W" reads a guard cell whose g is -inf and fails ``g[n] > g2`` like a closed cell.  So
the maps here make the search work along every border, and in particular where a missing column mask would wrap into the neighbouring row
and a missing guard row would read the chunk minima or the bytes in front of the state.

Yardsticks, as in test_stored_heuristic_gpu.py (whose launch helpers are used): the SAME call with ``passable = cost.clone()`` takes the
general stream (which still computes both coordinates) and must give the same bits in every output; the binary maps are also compared with
the CPU oracle, selection log included.  Every output buffer has guard bytes behind it.  Shapes 16x16, 32x32, 64x64; B = 1, 3, 65; the plain
kernel (nastar_forward_ex) and the ranked one (nastar_forward_levels).
"""
import ctypes

import numpy as np
import pytest

from test_stored_heuristic_gpu import POISON, _launch, _levels, _pair, _same_bits

pytestmark = pytest.mark.gpu

SIZES = (16, 32, 64)
BATCHES = (1, 3, 65)

_BANKS = {}


def _bank(W):
    """[(map [W, W] float32, start cell, goal cell, name)] -- computed once per size, shared, never modified"""
    if W in _BANKS:
        return _BANKS[W]
    rng = np.random.default_rng(7000 + W)
    L, M = W - 1, W // 2
    cases = []

    def add(m, s, g, name):
        cases.append((np.ascontiguousarray(m, dtype=np.float32), s[0] * W + s[1], g[0] * W + g[1], name))

    def rand_map(*keep):
        m = (rng.random((W, W)) > 0.2).astype(np.float32)
        for p in keep:
            m[p] = 1
        return m

    ones = np.ones((W, W), np.float32)
    # 1. all passable: opposite corners and the middles of opposite edges, both ways -- the frontier sweeps all four borders
    for a, b in (((0, 0), (L, L)), ((0, L), (L, 0)), ((0, M), (L, M)), ((M, 0), (M, L)), ((0, M - 1), (L, M)), ((M, 0), (M - 1, L))):
        add(ones, a, b, f"ones{a}{b}")
        add(ones, b, a, f"ones{b}{a}")
    # 2. a one-cell-wide corridor along each border, walked both ways, and the ring of all four
    for name, sl, a, b in (("top", (0, slice(None)), (0, 0), (0, L)), ("bottom", (L, slice(None)), (L, 0), (L, L)),
                           ("left", (slice(None), 0), (0, 0), (L, 0)), ("right", (slice(None), L), (0, L), (L, L))):
        m = np.zeros((W, W), np.float32)
        m[sl] = 1
        add(m, a, b, f"corridor_{name}")
        add(m, b, a, f"corridor_{name}_back")
    ring = np.zeros((W, W), np.float32)
    ring[0, :] = ring[L, :] = ring[:, 0] = ring[:, L] = 1
    add(ring, (0, 1), (L, L - 1), "ring")
    add(ring, (M, L), (M, 0), "ring_sides")
    # 3. the start on an obstacle in each corner and on each edge: its first step hands on g2 = 0.0 next to a guard row
    for k, s in enumerate(((0, 0), (0, L), (L, 0), (L, L), (0, M), (L, M - 1), (M, 0), (M + 1, L))):
        g = (L - s[0] if s[0] in (0, L) else M, L - s[1] if s[1] in (0, L) else M - 1)
        m = rand_map(g)
        m[s] = 0
        add(m, s, g, f"start_blocked{k}")
        m = ones.copy()
        m[s] = 0
        add(m, s, g, f"start_blocked_ones{k}")
    # 4. the goal in row 0 / row W-1 / column 0 / column W-1 (random obstacles; some are unsolvable: both streams agree on that too)
    for k, g in enumerate(((0, 3), (0, L - 2), (L, 2), (L, L - 4), (5, 0), (L - 3, 0), (4, L), (L - 6, L), (0, 0), (L, L), (0, L), (L, 0))):
        s = (M + (k % 3) - 1, M - (k % 2))
        add(rand_map(s, g), s, g, f"goal_border{k}")
    # 5. only column 0 and column W-1 are passable, joined along row 0 (and along row W-1): the shortest route runs up, across and down --
    #    a lane that wraps from column W-1 into column 0 of the next row (or back) finds a shortcut of one step
    for row, name in ((0, "u_top"), (L, "u_bottom")):
        m = np.zeros((W, W), np.float32)
        m[:, 0] = m[:, L] = m[row, :] = 1
        far = L - row
        add(m, (far, 0), (far, L), name)
        add(m, (far, L), (far, 0), name + "_back")
        add(m, (M, L), (M - 1, 0), name + "_mid")
    # ... and the two columns with nothing joining them: unsolvable unless a lane wraps
    m = np.zeros((W, W), np.float32)
    m[:, 0] = m[:, L] = 1
    add(m, (2, 0), (3, L), "two_columns")
    add(m, (L, L), (0, 0), "two_columns_back")
    # 6. one value other than +0.0 / 1.0 on a border: 0.5, 2.0, -1.0 and NaN send the map to a general stream (raw-bit keys or, for the
    #    signed ones, the order-preserving transform) on the same layout, beside its neighbours; -0.0 compares equal to 0.0 and keeps
    #    the stored-heuristic stream
    for k, v in enumerate(POISON):
        p = ((0, 2 + k), (L, 3 + k), (2 + k, 0), (4 + k, L), (0, L))[k]
        s, g = (1, 1), (L - 1, L - 1)
        m = rand_map(s, g)
        m[p] = v
        add(m, s, g, f"poison{v}")
    _BANKS[W] = cases
    return cases


def _batch(W, B, first=0):
    bank = _bank(W)
    m = np.empty((B, W, W), np.float32)
    s = np.zeros((B, W * W), np.float32)
    g = np.zeros((B, W * W), np.float32)
    names = []
    for b in range(B):
        mm, si, gi, name = bank[(first + b) % len(bank)]
        m[b] = mm
        s[b, si] = 1
        g[b, gi] = 1
        names.append(name)
    return m, s.reshape(B, W, W), g.reshape(B, W, W), names


# ---- 1. every border case, every shape, both kernels: the same bits as the general stream --------------------------------------------------
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("W", SIZES)
def test_border_maps_equal_the_general_stream(W, B):
    n = len(_bank(W))
    for first in (range(0, n, B) if B < n else (0, 11)):  # the small batches walk through the whole bank
        m, s, g, names = _batch(W, B, first)
        ex = _pair(m, s, g, (W, B, first, "ex"))
        lv = _pair(m, s, g, (W, B, first, "levels"), which="levels", levels=_levels(B, first))
        _same_bits(ex, lv, (W, B, first, "ex vs levels"))
        assert ex["summary"][0] == 1  # the completion flag came up


# ---- 2. the mixed batch: stored-heuristic maps and maps with one non-binary value side by side in one launch --------------------------------
@pytest.mark.parametrize("W", SIZES)
def test_mixed_batch_runs_both_streams_in_one_launch(W):
    bank = _bank(W)
    poison = [k for k, c in enumerate(bank) if c[3].startswith("poison")]
    assert len(poison) == len(POISON)
    B = 65
    m, s, g, names = _batch(W, B)
    for b in range(0, B, 2):  # every other map holds one of the POISON values (four of the five leave the stored-heuristic stream)
        mm, si, gi, _ = bank[poison[(b // 2) % len(poison)]]
        m[b] = mm
        s[b] = 0
        g[b] = 0
        s[b].reshape(-1)[si] = 1
        g[b].reshape(-1)[gi] = 1
    ex = _pair(m, s, g, (W, "mixed"))
    lv = _pair(m, s, g, (W, "mixed levels"), which="levels", levels=_levels(B, 3))
    _same_bits(ex, lv, (W, "mixed ex vs levels"))


# ---- 3. against the CPU oracle, selection log included (the logging instantiation) -----------------------------------------------------------
@pytest.mark.parametrize("W", SIZES)
def test_border_maps_equal_the_oracle(W):
    from oracle import oracle as O
    B = len(_bank(W))
    m, s, g, names = _batch(W, B)
    keep = np.array([not n.startswith("poison") for n in names])
    got = _pair(m, s, g, (W, "log"), log=True)
    o = O.forward(m[keep], s[keep], g[keep], m[keep], 0.5, W * W, mode="sm", want_log=True)
    it = got["iters"][keep]
    assert np.array_equal(it, o.iters)
    assert np.array_equal(got["histories"].reshape(B, W, W)[keep], o.histories)
    assert np.array_equal(got["paths"].reshape(B, W, W)[keep], o.paths)
    assert np.array_equal(got["status"][keep] != 0, o.map_status != 0)
    log = got["sel_log"].reshape(B, W * W)[keep]
    for b in range(int(keep.sum())):
        assert np.array_equal(log[b, :it[b]], o.sel_log[b, :it[b]]), names[b]
    # what the maps were built for: the U routes go all the way round (3 W - 4 cells when both corners are cut), the two lone columns stay apart
    by = {n: b for b, n in enumerate(names)}
    for n in ("u_top", "u_top_back", "u_bottom", "u_bottom_back"):
        assert got["status"][by[n]] == 0 and got["paths"].reshape(B, -1)[by[n]].sum() >= 3 * W - 4, n
    for n in ("two_columns", "two_columns_back"):
        assert got["status"][by[n]] != 0, n


# ---- 4. other g_ratio (the stream with both products) and the routes entry on the border maps ---------------------------------------------
@pytest.mark.parametrize("W", SIZES)
def test_border_maps_g_ratio_and_routes(W):
    m, s, g, names = _batch(W, 65, first=5)
    _pair(m, s, g, (W, 0.3), g_ratio=0.3)
    _pair(m, s, g, (W, 0.8, "levels"), which="levels", levels=_levels(65, 9), g_ratio=0.8)
    _pair(m, s, g, (W, "routes"), routes=True, marks=True)


# ---- 5. the layout keeps the resident maps per CU ----------------------------------------------------------------------------------------------
def test_occupancy_and_lds_bytes():
    from neural_astar import _native
    lib = _native.load()
    n = ctypes.c_int(-1)
    assert lib.nastar_debug_occupancy(32, 32, ctypes.addressof(n)) == 16
    assert n.value == 10240  # 256 + 8192 + 256 + 512 + 1024 = 160 KiB / 16
    assert lib.nastar_debug_occupancy(64, 64, ctypes.addressof(n)) == 4
    assert n.value == 512 + 32768 + 512 + 2048 + 4096
    assert lib.nastar_debug_occupancy(16, 16, ctypes.addressof(n)) >= 16
    assert n.value == 128 + 2048 + 128 + 512 + 256
