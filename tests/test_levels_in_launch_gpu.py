"""GPU tests (-m gpu) of the search launch that places its maps by their levels itself (include/nastar_levels.h).

Where a map is searched never changes what is computed: every output of the ranked launch must be bit-equal to nastar_forward_ex without an
order and to the CPU oracle; the placement itself is observed through nastar_placement_slots (the same device function, one workgroup per
slot) and must equal the numpy restatement of the rule (tests/placement_rule.py) exactly.
"""
import ctypes

import numpy as np
import pytest
import torch

import placement_rule as PR
from test_levels_in_launch import REFUSALS, level_args

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- 1. the placement against the restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", PR.BATCH_SIZES)
def test_slots_equal_the_restatement_and_are_a_permutation(B):
    from neural_astar import _native
    lib = _native.load()
    for name, lv in PR.level_sets(B).items():
        lvt = _t(lv)
        out = torch.full((B,), -7, dtype=torch.int32, device=_dev())
        assert lib.nastar_placement_slots(lvt.data_ptr(), B, out.data_ptr(), _stream()) == 0
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert PR.is_permutation(got, B), (B, name)
        assert np.array_equal(got, PR.slots(lv)), (B, name)


# ---- 2. / 3. outputs of the ranked launch ----------------------------------------------------------------------------------------------
def _problems(B, W, seed):
    from neural_astar.utils import synthetic as syn
    pr = syn.random_obstacle_maps(B, W, W, 0.2, seed=seed)
    return tuple(np.ascontiguousarray(x[:, 0]) for x in (pr.map_designs, pr.start_maps, pr.goal_maps))


def _launch(which, m, s, g, levels=None, cost=None):
    """one launch through ctypes -> (histories, paths, iters, status, packed, summary) as numpy; `which` = "ex" (no order) or "levels" """
    from neural_astar import _native, ops
    lib = _native.load()
    dev = _dev()
    B, H, W = m.shape
    mt, st, gt = _t(m), _t(s), _t(g)
    ct = mt if cost is None else _t(cost)
    hist = torch.full((B, H, W), -1.0, dtype=torch.float32, device=dev)
    paths = torch.full((B, H, W), -1, dtype=torch.int64, device=dev)
    it = torch.full((B,), -1, dtype=torch.int32, device=dev)
    stt = torch.full((B,), -1, dtype=torch.int32, device=dev)
    packed = torch.zeros((B, 2 * ((H * W + 7) // 8)), dtype=torch.uint8, device=dev)
    summ = torch.zeros(ops.SUMMARY_WORDS, dtype=torch.int32, device=dev)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    head = (ct.data_ptr(), st.data_ptr(), gt.data_ptr(), mt.data_ptr(), B, H, W, 0.5, H * W, hist.data_ptr(), paths.data_ptr(), None, it.data_ptr(),
            stt.data_ptr(), packed.data_ptr(), None, 0, 0)
    tail = (summ.data_ptr(), counter.data_ptr(), _stream())
    if which == "levels":
        lvt = _t(levels)
        rc = lib.nastar_forward_levels(*head, lvt.data_ptr(), *tail)
    else:
        rc = lib.nastar_forward_ex(*head, None, None, *tail)
    assert rc == 0, (which, rc)
    torch.cuda.synchronize()
    assert int(counter[0]) == 0  # (B completions bring the cell back to 0)
    return tuple(x.cpu().numpy() for x in (hist, paths, it, stt, packed, summ))


@pytest.fixture(scope="module")
def searched():
    """{W: (problem, nastar_forward_ex outputs, oracle)} for B = 130 (three blocks of 44 / 43 / 43 maps), computed once"""
    from oracle import oracle as O
    out = {}
    for W in (16, 32, 64):
        m, s, g = _problems(130, W, seed=40 + W)
        out[W] = ((m, s, g), _launch("ex", m, s, g), O.forward(m, s, g, m, 0.5, W * W, mode="sm"))
    return out


@pytest.mark.parametrize("W", [16, 32, 64])
@pytest.mark.parametrize("kind", ["random", "all_equal"])
def test_ranked_launch_outputs_equal_the_plain_launch_and_the_oracle(searched, W, kind):
    (m, s, g), ex, o = searched[W]
    B = m.shape[0]
    lv = np.random.default_rng(W).integers(0, 9, B).astype(np.int32) if kind == "random" else np.full(B, 5, np.int32)
    got = _launch("levels", m, s, g, lv)
    for name, a, b in zip(("histories", "paths", "iters", "status", "packed", "summary"), got, ex):
        assert np.array_equal(a, b), (W, kind, name)
    hist, paths, it, st = got[:4]
    assert np.array_equal(hist, o.histories) and np.array_equal(paths, o.paths) and np.array_equal(it, o.iters), (W, kind)
    assert np.array_equal(st != 0, o.map_status != 0), (W, kind)
    assert got[5][0] == 1  # the completion flag came up


def test_unsolvable_map_reports_like_the_plain_launch():
    from neural_astar import ops
    W, B = 32, 130
    m = np.ones((B, W, W), np.float32)
    s, g = np.zeros_like(m), np.zeros_like(m)
    s[:, 0, 0] = 1
    g[:, W - 1, W - 1] = 1
    m[77, W - 3, :] = 0  # map 77: its goal is walled in
    lv = np.random.default_rng(3).integers(0, 60, B).astype(np.int32)
    ex = _launch("ex", m, s, g)
    got = _launch("levels", m, s, g, lv)
    for name, a, b in zip(("histories", "paths", "iters", "status", "packed", "summary"), got, ex):
        assert np.array_equal(a, b), name
    st, summ = got[3], got[5]
    assert st[77] == ops.STATUS_UNSOLVABLE and (np.delete(st, 77) == 0).all()
    assert summ[0] == 1 and summ[ops.STATUS_UNSOLVABLE] == 1 and summ[1:].sum() == 1


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("over,rc,in_launch", REFUSALS)
def test_refusals_come_before_any_launch(over, rc, in_launch):
    """(the same table runs without a device in tests/test_levels_in_launch.py: refused on the arguments alone; here, on the device, the
    pointers are never dereferenced either -- nothing faults, nothing is queued)"""
    from neural_astar import _native
    lib = _native.load()
    a = level_args(**over)
    assert lib.nastar_forward_levels(*a.values()) == rc
    assert lib.nastar_levels_in_launch(a["H"], a["W"], a["flags"], int(a["sel_log_out"] is not None)) == in_launch
    torch.cuda.synchronize()


# ---- 5. the module does not sort where the launch ranks ------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,sorts", [(32, 32, 0), (20, 44, 1)])
def test_forward_with_levels_calls_the_sort_only_where_the_launch_cannot_rank(H, W, sorts):
    from neural_astar import _native, ops
    from neural_astar.planner import VanillaAstar
    fl = _native.load_fastlane()
    assert fl is not None, "lib/_nastar_fastlane.so missing: __graft_entry__.build() builds it"
    lib = _native.load()
    calls = {"n": 0}
    sort_t = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p)

    @sort_t
    def counting(levels, B, order_out, stream):
        calls["n"] += 1
        return lib.nastar_placement_from_levels(levels, B, order_out, stream)

    # solvable by construction (the call checks): single-cell obstacles on the odd/odd lattice never close an 8-connected route, and
    # starts and goals sit on even/even cells
    rng = np.random.default_rng(9)
    B = 130
    mm = np.ones((B, 1, H, W), np.float32)
    mm[:, :, 1::2, 1::2] = (rng.random((B, 1, H // 2, W // 2)) > 0.6).astype(np.float32)
    ss, gg = np.zeros_like(mm), np.zeros_like(mm)
    for b in range(B):
        ss[b, 0, 2 * rng.integers(0, H // 2), 2 * rng.integers(0, W // 2)] = 1
        gg[b, 0, 2 * rng.integers(0, H // 2), 2 * rng.integers(0, W // 2)] = 1
    m, s, g = _t(mm), _t(ss), _t(gg)
    lv = _t(rng.integers(0, 50, B).astype(np.int32))
    va = VanillaAstar().to(_dev()).eval()
    _native._fastlane = (fl[0], fl[1], ctypes.cast(counting, ctypes.c_void_p).value)
    try:
        with torch.no_grad():
            plain = va(m, s, g)
            assert calls["n"] == 0
            ops.attach_levels(s, lv)
            hinted = va(m, s, g)
            torch.cuda.synchronize()
            assert calls["n"] == sorts
            assert s.placement_order.order is None  # nothing was sorted in Python either
    finally:
        _native._fastlane = fl
        del s.placement_order
    assert torch.equal(plain.histories, hinted.histories) and torch.equal(plain.paths, hinted.paths)
