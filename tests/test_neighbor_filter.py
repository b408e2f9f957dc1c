"""CPU: DifferentiableAstar.neighbor_filter -> the kernels' 9-bit neighbourhood mask (orientation, validation, caching), the argument checks
of the masked C entry points, and the reference vectors of tests/golden/neighbors/."""
import numpy as np
import pytest
import torch

import neighbor_golden as NG
from neural_astar import _native, ops
from neural_astar.planner.differentiable_astar import DifferentiableAstar

VN = [[0, 1, 0], [1, 0, 1], [0, 1, 0]]


def _set(m, filt):
    with torch.no_grad():
        m.neighbor_filter.copy_(torch.tensor(filt, dtype=torch.float32).reshape(1, 1, 3, 3))


def _lane_offsets(mask):
    """the kernels' gate restated (csrc/nastar_device.hip.h: neighbour_enabled): lane j owns offset cell k = j + (j >= 4) of the 3x3 stencil in
    raster order, and filter cell 8 - k opens it"""
    out = set()
    for j in range(8):
        k = j + (j >= 4)
        if (mask >> (8 - k)) & 1:
            out.add((k // 3 - 1, k % 3 - 1))
    return out


def _conv_offsets(filt):
    """what the reference's expand() (conv2d with padding 1) opens around a one-hot at the centre of a 5x5 map"""
    x = torch.zeros(1, 1, 5, 5)
    x[0, 0, 2, 2] = 1
    y = torch.nn.functional.conv2d(x, torch.tensor(filt, dtype=torch.float32).reshape(1, 1, 3, 3), padding=1)[0, 0]
    return {(int(r) - 2, int(c) - 2) for r, c in zip(*torch.nonzero(y, as_tuple=True))}


def test_mask_encoding_of_the_named_neighbourhoods():
    m = DifferentiableAstar()
    assert m.neighbor_mask() is None  # the default filter keeps the Moore-8 kernels
    assert NG.mask_of(m.neighbor_filter[0, 0].numpy()) == ops.NEIGHBORS_MOORE8 == 0x1EF
    _set(m, VN)
    assert m.neighbor_mask() == ops.NEIGHBORS_VON_NEUMANN == 0x0AA


@pytest.mark.parametrize("seed", range(8))
def test_orientation_matches_conv2d(seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    filt = (rng.random((3, 3)) < 0.5).astype(np.float32)
    filt[1, 1] = 0
    m = DifferentiableAstar()
    _set(m, filt)
    mask = m.neighbor_mask()
    mask = ops.NEIGHBORS_MOORE8 if mask is None else mask
    assert _lane_offsets(mask) == _conv_offsets(filt)
    # the point reflection: top-middle opens the cell one row BELOW
    top = np.zeros((3, 3), np.float32)
    top[0, 1] = 1
    assert _conv_offsets(top) == {(1, 0)} and _lane_offsets(NG.mask_of(top)) == {(1, 0)}


@pytest.mark.parametrize("bad", [
    [[0.5, 1, 1], [1, 0, 1], [1, 1, 1]],
    [[1, 1, 1], [1, 1, 1], [1, 1, 1]],
    [[2, 0, 0], [0, 0, 0], [0, 0, 0]],
    [[-1, 0, 0], [0, 0, 0], [0, 0, 0]],
    [[float("nan"), 1, 1], [1, 0, 1], [1, 1, 1]],
])
def test_unsupported_filters_are_refused_by_name(bad):
    m = DifferentiableAstar()
    _set(m, bad)
    with pytest.raises(NotImplementedError, match="neighbor_filter"):
        m.neighbor_mask()
    with pytest.raises(NotImplementedError, match="neighbor_filter"):  # every call, not only the first
        m.neighbor_mask()
    x = torch.ones(1, 1, 8, 8)
    with pytest.raises(NotImplementedError, match="neighbor_filter"):  # before anything else looks at the inputs
        m(x, x, x, x)


def test_unsupported_shape_is_refused():
    m = DifferentiableAstar()
    m.neighbor_filter = torch.nn.Parameter(torch.ones(1, 1, 5, 5), requires_grad=False)
    with pytest.raises(NotImplementedError, match=r"\(1, 1, 5, 5\)"):
        m.neighbor_mask()


def test_the_cache_sees_every_versioned_change():
    m = DifferentiableAstar()
    assert m.neighbor_mask() is None
    _set(m, VN)  # copy_ under no_grad
    assert m.neighbor_mask() == 0x0AA
    with torch.no_grad():
        m.neighbor_filter.fill_(1.0)
        m.neighbor_filter[0, 0, 1, 1] = 0
    assert m.neighbor_mask() is None
    sd = DifferentiableAstar().state_dict()
    sd["neighbor_filter"] = torch.tensor(VN, dtype=torch.float32).reshape(1, 1, 3, 3)
    m.load_state_dict(sd)
    assert m.neighbor_mask() == 0x0AA
    m.neighbor_filter = torch.nn.Parameter(torch.tensor([[1.0, 1, 0], [1, 0, 0], [0, 0, 0]]).reshape(1, 1, 3, 3), requires_grad=False)
    assert m.neighbor_mask() == 0b000001011
    m = m.to(torch.float64)  # .to() keeps the values: the cached mask carries over
    assert m.neighbor_mask() == 0b000001011


def test_masked_entry_points_check_their_arguments():
    lib = _native.load()
    one = 16  # any non-NULL address: every call below is refused before a pointer is dereferenced
    assert lib.nastar_version() >= 700
    ws = 1 << 20
    for bad in (0x1FF, 0x010, 0x200, 0x1EF | (1 << 12), 0xFFFFFFFF):
        assert lib.nastar_forward_ex_masked(one, one, one, one, 1, 8, 8, 0.5, 64, one, one, None, one, one, None, None, 0, 0, None, None, None, None,
                                            bad, None) == _native.NASTAR_ERR_UNSUPPORTED, hex(bad)
        assert lib.nastar_forward_batchloop_finish_masked(one, one, one, one, 2, 8, 8, 0.5, 64, one, one, None, one, one, one, ws, bad,
                                                          None) == _native.NASTAR_ERR_UNSUPPORTED, hex(bad)
        assert lib.nastar_backward_replay_ordered_masked(one, None, None, None, one, one, one, one, one, 1, 8, 8, 0.5, 64, one, None, one, one, ws, 0,
                                                         None, bad, None) == _native.NASTAR_ERR_UNSUPPORTED, hex(bad)
    for good in (0x1EF, 0x0AA, 0x000, 0x00B):
        assert lib.nastar_forward_ex_masked(None, one, one, one, 1, 8, 8, 0.5, 64, one, one, None, one, one, None, None, 0, 0, None, None, None, None,
                                            good, None) == _native.NASTAR_ERR_NULL
        assert lib.nastar_forward_ex_masked(one, one, one, one, 0, 8, 8, 0.5, 64, one, one, None, one, one, None, None, 0, 0, None, None, None, None,
                                            good, None) == _native.NASTAR_ERR_BAD_SHAPE
        assert lib.nastar_forward_ex_masked(one, one, one, one, 1, 8, 8, 0.5, 64, one, one, None, one, one, None, None, 0, 8, None, None, None, None,
                                            good, None) == _native.NASTAR_ERR_UNSUPPORTED  # unknown flag bits stay refused
        assert lib.nastar_forward_batchloop_finish_masked(one, one, one, one, 2, 8, 8, 0.5, 64, one, one, None, one, one, None, 0, good,
                                                          None) == _native.NASTAR_ERR_NULL
        assert lib.nastar_backward_replay_ordered_masked(None, None, None, None, one, one, one, one, one, 1, 8, 8, 0.5, 64, one, None, one, one, ws,
                                                         0, None, good, None) == _native.NASTAR_ERR_NULL


def test_header_names_the_encoding():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nastar.h")).read()
    assert int(re.search(r"#define NASTAR_NEIGHBORS_MOORE8 (0x[0-9A-Fa-f]+)", hdr).group(1), 16) == ops.NEIGHBORS_MOORE8
    assert int(re.search(r"#define NASTAR_NEIGHBORS_VON_NEUMANN (0x[0-9A-Fa-f]+)", hdr).group(1), 16) == ops.NEIGHBORS_VON_NEUMANN


def test_reference_vectors_hold_the_issue_table():
    g = NG.load("fixture64_vn_g050")
    assert NG.mask_of(g.filter) == 0x0AA
    assert int(g.histories[0].sum()) == 3395 and int(g.paths[0].sum()) == 127  # Moore-8: 1169 / 88
    g = NG.load("fixture64_dr_g050")
    assert int(g.histories[0].sum()) == 1169 and int(g.paths[0].sum()) == 88
    names = NG.names()
    assert {"rand32_asym_g050", "rand32_vn_ucost_g020", "rand20x45_vn_ucost_g050", "rand80_asym_ucost_g050", "grad_rand32_vn_train_T025",
            "grad_rand80_asym_train_T025"} <= set(names)
    for n in names:
        g = NG.load(n)
        B = g.histories.shape[0]
        assert g.sel_log.shape == (B, g.t_batch + 1)
        # the reference closes exactly the cells it selects before the goal: the log and the histories agree
        for b in range(B):
            goal = int(g.goal_maps[b].reshape(-1).argmax())
            row = g.sel_log[b]
            hit = np.flatnonzero(row == goal)
            last = int(hit[0]) + 1 if hit.size else row.size
            assert set(row[:last].tolist()) <= set(np.flatnonzero(g.histories[b].reshape(-1)).tolist())


def test_a_trace_uses_the_cached_mask_and_refuses_a_changed_filter(monkeypatch):
    m = DifferentiableAstar()
    _set(m, VN)
    assert m.neighbor_mask() == 0x0AA  # read (and cached) outside the trace
    monkeypatch.setattr(torch.compiler, "is_compiling", lambda: True)
    assert m.neighbor_mask() == 0x0AA  # unchanged: the cached mask, no read
    _set(m, [[1, 1, 0], [1, 0, 0], [0, 0, 0]])
    with pytest.raises(RuntimeError, match="neighbor_filter changed"):
        m.neighbor_mask()
    monkeypatch.undo()
    assert m.neighbor_mask() == 0b000001011
