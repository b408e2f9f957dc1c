"""CPU: the shortest-path mask and its blackbox gradient for maps of up to 1179648 cells (include/nastar_path_masks_tiled.h,
``ops.shortest_paths_tiled``, the planners' ``shortest_paths_tiled``) -- everything that needs no GPU.

1. the twelfth header against ``_native.PATH_MASK_TILED_SIGNATURES``; the library's symbols, abi, limit and workspace sizes;
2. every refusal the two entry points make before any HIP call, and their order;
3. the Python refusals made without a device;
4. the definition is tests/path_masks_oracle.py, unchanged: this file adds no numpy definition of its own.
"""
import inspect

import numpy as np
import pytest
import torch

import path_masks_oracle as PO
from test_fields import _defines, _prototypes

LIMIT = 1179648
NAMES = ["nastar_path_masks_tiled", "nastar_path_masks_tiled_abi", "nastar_path_masks_tiled_backward",
         "nastar_path_masks_tiled_backward_workspace_bytes", "nastar_path_masks_tiled_max_cells", "nastar_path_masks_tiled_workspace_bytes"]
ARGS = ["cost", "goal", "passable", "start_idx", "B", "H", "W", "neighbor_mask", "path_out", "path_cost_out", "status_out", "workspace",
        "workspace_bytes", "max_rounds", "rounds_out", "stream"]
BACK_ARGS = ["cost", "goal", "passable", "start_idx", "grad_path", "path_fwd", "status_fwd", "B", "H", "W", "neighbor_mask", "lambda", "min_cost",
             "grad_cost_out", "status_out", "workspace", "workspace_bytes", "max_rounds", "rounds_out", "stream"]
BAD_SHAPE, UNSUPPORTED, NULL, WORKSPACE = 1, 2, 5, 6


# ---- 1: header, binding, library ----------------------------------------------------------------------------------------------------------------------
def test_twelfth_header_and_path_mask_tiled_signatures_agree():
    from neural_astar import _native
    protos = _prototypes("nastar_path_masks_tiled.h")
    assert sorted(protos) == sorted(_native.PATH_MASK_TILED_SIGNATURES) == NAMES
    for name, (ret, args) in protos.items():
        assert _native.PATH_MASK_TILED_SIGNATURES[name] == ret + " " + "".join(k for k, _ in args), name
    assert [n for _, n in protos["nastar_path_masks_tiled"][1]] == ARGS
    assert [n for _, n in protos["nastar_path_masks_tiled_backward"][1]] == BACK_ARGS
    # a table of its own; nastar.h and the other tables are what they were
    for table in (_native.SIGNATURES, _native.ROUTE_SIGNATURES, _native.FIELD_SIGNATURES, _native.TILED_FIELD_SIGNATURES, _native.FIELD_GRAD_SIGNATURES,
                  _native.FIELD_GRAD_TILED_SIGNATURES, _native.FIELD_ROUTE_SIGNATURES, _native.PATH_MASK_SIGNATURES, _native.VERDICT_SIGNATURES):
        assert not set(_native.PATH_MASK_TILED_SIGNATURES) & set(table)
    assert len(_prototypes("nastar.h")) == len(_native.SIGNATURES) == 74 and len(_prototypes("nastar_path_masks.h")) == 4
    new = _defines("nastar_path_masks_tiled.h")
    assert new["NASTAR_PATH_MASKS_TILED_ABI"] == 1 and "NASTAR_VERSION" not in new and _defines("nastar.h")["NASTAR_VERSION"] == 800
    assert not [k for k in new if k.startswith("NASTAR_ERR_")]      # no new status code
    assert (_native.NASTAR_ERR_BAD_SHAPE, _native.NASTAR_ERR_UNSUPPORTED, _native.NASTAR_ERR_NULL, _native.NASTAR_ERR_WORKSPACE) == (
        BAD_SHAPE, UNSUPPORTED, NULL, WORKSPACE)


def test_library_exports_the_tiled_path_mask_symbols_and_sizes_its_workspace():
    from neural_astar import _native, ops
    lib = _native.load()
    for sym in NAMES:
        assert hasattr(lib, sym), sym
    assert lib.nastar_path_masks_tiled_abi() == 1
    assert lib.nastar_path_masks_tiled_max_cells() == ops.PATH_MASKS_TILED_MAX_CELLS == lib.nastar_fields_tiled_max_cells() == LIMIT
    assert len(lib.nastar_path_masks_tiled.argtypes) == 16 and len(lib.nastar_path_masks_tiled_backward.argtypes) == 20
    assert {"shortest_paths_tiled", "path_masks_tiled", "path_masks_tiled_backward", "PATH_MASKS_TILED_MAX_CELLS"} <= set(ops.__all__)
    fwd, back = lib.nastar_path_masks_tiled_workspace_bytes, lib.nastar_path_masks_tiled_backward_workspace_bytes
    for size in (fwd, back):
        for B, H, W in [(0, 8, 8), (-1, 8, 8), (1, 0, 8), (1, 8, 0), (1, 8, -5), (1, 1025, 1152), (1, 1, LIMIT + 1), (1, 65536, 65536),
                        (1 << 24, 65, 64)]:           # (the last: two tiles per map, more than 2^24 tiles)
            assert size(B, H, W) == 0, (B, H, W)
    for B, H, W in [(1, 1, 1), (3, 64, 64), (2, 129, 128), (5, 130, 259), (1, 1024, 1152), (2, 1, LIMIT), (1 << 24, 64, 64)]:
        field = lib.nastar_cost_to_go_tiled_workspace_bytes(B, H, W)
        assert field > 0 and fwd(B, H, W) >= 4 * B * H * W + 4 * B + field, (B, H, W)     # the field, the relaxation's status, its words
        assert back(B, H, W) >= fwd(B, H, W) + 4 * B * H * W, (B, H, W)                   # ... and the perturbed costs
        assert fwd(B, H, W) % 4 == 0 and back(B, H, W) % 4 == 0


# ---- 2: refusals, made before any HIP call --------------------------------------------------------------------------------------------------------------
def _args(**over):
    p = 0x10000  # never dereferenced: every call below is refused on its arguments
    a = dict(cost=p, goal=p, passable=p, start_idx=p, B=2, H=129, W=128, neighbor_mask=0x1EF, path_out=p, path_cost_out=None, status_out=p,
             workspace=p, workspace_bytes=0, max_rounds=0, rounds_out=None, stream=None)
    assert list(a) == ARGS
    a.update(over)
    return a


def _back_args(**over):
    p = 0x10000
    a = dict(cost=p, goal=p, passable=p, start_idx=p, grad_path=p, path_fwd=p, status_fwd=p, B=2, H=129, W=128, neighbor_mask=0x1EF, lambda_=20.0,
             min_cost=2.0 ** -10, grad_cost_out=p, status_out=None, workspace=p, workspace_bytes=0, max_rounds=0, rounds_out=None, stream=None)
    assert [k.rstrip("_") for k in a] == BACK_ARGS
    a.update(over)
    return a


# every base call ends in WORKSPACE (workspace_bytes = 0): whatever is refused with another code was refused BEFORE the workspace was looked at
SHARED_REFUSALS = [
    (dict(), WORKSPACE),
    (dict(workspace_bytes=1 << 40, workspace=0x10002), WORKSPACE),         # large enough, off a 4-byte boundary
    (dict(cost=None), NULL), (dict(goal=None), NULL), (dict(passable=None), NULL), (dict(start_idx=None), NULL), (dict(workspace=None), NULL),
    (dict(B=0), BAD_SHAPE), (dict(H=0), BAD_SHAPE), (dict(W=-1), BAD_SHAPE), (dict(B=-3), BAD_SHAPE), (dict(max_rounds=-1), BAD_SHAPE),
    (dict(neighbor_mask=0x1FF), UNSUPPORTED), (dict(neighbor_mask=0x200), UNSUPPORTED),
    (dict(neighbor_mask=0x010, cost=None), UNSUPPORTED),                   # the mask is looked at first
    (dict(cost=None, B=0), NULL), (dict(workspace=None, max_rounds=-1), NULL),   # a NULL before the shape
    (dict(B=0, H=1025, W=1152), BAD_SHAPE), (dict(max_rounds=-1, H=1025, W=1152), BAD_SHAPE),   # the shape before the limit
    (dict(H=1025, W=1152), UNSUPPORTED), (dict(H=1, W=LIMIT + 1), UNSUPPORTED), (dict(H=65536, W=65536), UNSUPPORTED),   # the limit before the workspace
    (dict(B=1 << 24, H=65, W=64), UNSUPPORTED),                            # more than 2^24 tiles
    (dict(H=1024, W=1152), WORKSPACE), (dict(H=1, W=LIMIT), WORKSPACE)]   # AT the limit: accepted as far as the workspace


@pytest.mark.parametrize("over,rc", SHARED_REFUSALS + [(dict(path_out=None), NULL), (dict(status_out=None), NULL), (dict(path_out=None, H=0), NULL)])
def test_path_masks_tiled_refuses_bad_arguments_without_a_device(over, rc):
    from neural_astar import _native
    lib = _native.load()
    assert lib.nastar_path_masks_tiled(*_args(**over).values()) == rc
    assert lib.nastar_path_masks_tiled(*_args(path_cost_out=0x10000, **over).values()) == rc
    a = _args(**over)
    need = lib.nastar_path_masks_tiled_workspace_bytes(a["B"], a["H"], a["W"])
    if need and "workspace_bytes" not in over:                                # one byte short is still short
        assert lib.nastar_path_masks_tiled(*_args(**dict(over, workspace_bytes=need - 1)).values()) == rc
    assert lib.nastar_last_error() == b""


@pytest.mark.parametrize("over,rc", SHARED_REFUSALS + [
    (dict(grad_path=None), NULL), (dict(path_fwd=None), NULL), (dict(status_fwd=None), NULL), (dict(grad_cost_out=None), NULL),
    (dict(lambda_=0.0), UNSUPPORTED), (dict(lambda_=-1.0), UNSUPPORTED), (dict(lambda_=float("inf")), UNSUPPORTED),
    (dict(lambda_=float("nan")), UNSUPPORTED),
    (dict(lambda_=1e-45), UNSUPPORTED),                                    # a denormal: its fp32 reciprocal is not finite
    (dict(min_cost=0.0), UNSUPPORTED), (dict(min_cost=-0.5), UNSUPPORTED), (dict(min_cost=float("inf")), UNSUPPORTED),
    (dict(min_cost=float("nan")), UNSUPPORTED),
    (dict(lambda_=0.0, H=1025, W=1152), UNSUPPORTED),
    (dict(lambda_=0.0, workspace_bytes=1 << 40), UNSUPPORTED),             # the step before the workspace (which would pass here)
    (dict(lambda_=0.0, B=0), BAD_SHAPE), (dict(min_cost=0.0, max_rounds=-1), BAD_SHAPE),   # the shape before the step
    (dict(min_cost=0.0, grad_path=None), NULL), (dict(lambda_=float("nan"), neighbor_mask=0x010), UNSUPPORTED)])
def test_path_masks_tiled_backward_refuses_bad_arguments_without_a_device(over, rc):
    from neural_astar import _native
    lib = _native.load()
    assert lib.nastar_path_masks_tiled_backward(*_back_args(**over).values()) == rc
    assert lib.nastar_path_masks_tiled_backward(*_back_args(status_out=0x10000, **over).values()) == rc
    a = _back_args(**over)
    need = lib.nastar_path_masks_tiled_backward_workspace_bytes(a["B"], a["H"], a["W"])
    if need and "workspace_bytes" not in over:
        assert lib.nastar_path_masks_tiled_backward(*_back_args(**dict(over, workspace_bytes=need - 1)).values()) == rc
        # the forward's size is not enough for the backward
        short = lib.nastar_path_masks_tiled_workspace_bytes(a["B"], a["H"], a["W"])
        assert lib.nastar_path_masks_tiled_backward(*_back_args(**dict(over, workspace_bytes=short)).values()) == rc
    assert lib.nastar_last_error() == b""


# ---- 3: Python refusals without a device ------------------------------------------------------------------------------------------------------------------
def test_ops_and_planners_refuse_before_a_launch():
    from neural_astar import ops
    from neural_astar.planner import NeuralAstar, VanillaAstar
    from neural_astar.planner.differentiable_astar import DifferentiableAstar
    m = torch.ones(2, 1, 8, 8)
    idx = torch.zeros(2, dtype=torch.int32)
    for kw in (dict(), dict(lambda_=20.0)):
        with pytest.raises(RuntimeError, match="HIP device"):
            ops.shortest_paths_tiled(m, m, m, m, **kw)
        with pytest.raises(RuntimeError, match="HIP device"):
            DifferentiableAstar().shortest_paths_tiled(m, m, m, m, **kw)
        with pytest.raises(RuntimeError, match="HIP device"):
            VanillaAstar().shortest_paths_tiled(m, m, m, **kw)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.path_masks_tiled(m, m, m, idx)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.path_masks_tiled_backward(m, m, m, idx, m, m, idx, 20.0)
    above = torch.ones(1, 1, 1, 1).expand(1, 1, 129, 128)                   # above the one-workgroup limit: the tiled calls get as far as the device
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.shortest_paths_tiled(above, above, above, above)
    with pytest.raises(ValueError, match="share one"):
        ops.shortest_paths_tiled(m, m, torch.ones(2, 1, 8, 9), m)
    with pytest.raises(TypeError, match="float32"):
        ops.shortest_paths_tiled(m.double(), m, m.double(), m.double())
    with pytest.raises(ValueError, match="neighbor_mask"):
        ops.shortest_paths_tiled(m, m, m, m, neighbor_mask=0x1FF)
    for bad in (torch.ones(2, 3, 8, 8), torch.ones(2, 1, 8, 9), torch.ones(1, 1, 8, 8), torch.zeros(2, 2, dtype=torch.int64), torch.ones(2, 64)):
        with pytest.raises(ValueError, match="start"):
            ops.shortest_paths_tiled(m, bad, m, m)
        with pytest.raises(ValueError, match="start"):
            ops.path_masks_tiled(m, m, m, bad)
    for bad in (None, [[0]], m.bool()):
        with pytest.raises((TypeError, ValueError), match="start"):
            ops.shortest_paths_tiled(m, bad, m, m)
    for bad in (0, 0.0, -1.0, float("inf"), float("nan"), True, "20", 1e-46, 1e39, torch.tensor(20.0)):
        with pytest.raises(ValueError, match="lambda_"):
            ops.shortest_paths_tiled(m, m, m, m, lambda_=bad)
        with pytest.raises(ValueError, match="lambda_"):
            NeuralAstar(encoder_arch="CNN").shortest_paths_tiled(m, m, m, lambda_=bad)
        with pytest.raises(ValueError, match="lambda_"):
            ops.path_masks_tiled_backward(m, m, m, idx, m, m, idx, bad)
    for bad in (0, -0.25, float("inf"), float("nan"), None, False, 1e-46):
        with pytest.raises(ValueError, match="min_cost"):
            ops.shortest_paths_tiled(m, m, m, m, min_cost=bad)
        with pytest.raises(ValueError, match="min_cost"):
            NeuralAstar(encoder_arch="CNN").shortest_paths_tiled(m, m, m, lambda_=20.0, min_cost=bad)
    for bad in (0, -1, True, 2.0):
        with pytest.raises(ValueError, match="max_rounds"):
            ops.path_masks_tiled(m, m, m, idx, max_rounds=bad)
    huge = torch.ones(1, 1, 1, 1).expand(1, 1, 1025, 1152)
    for call in (lambda: ops.shortest_paths_tiled(huge, huge, huge, huge), lambda: ops.shortest_paths_tiled(huge, huge, huge, huge, lambda_=1.0),
                 lambda: ops.path_masks_tiled(huge, huge, huge, idx[:1]),
                 lambda: ops.path_masks_tiled_backward(huge, huge, huge, idx[:1], huge, huge, idx[:1], 20.0),
                 lambda: VanillaAstar().shortest_paths_tiled(huge, huge, huge)):
        with pytest.raises(NotImplementedError, match=str(LIMIT)):
            call()
    # the one-workgroup calls refuse above 16384 cells exactly as before
    for call in (lambda: ops.shortest_paths(above, above, above, above), lambda: ops.path_masks(above, above, above, idx[:1])):
        with pytest.raises(NotImplementedError, match="16384"):
            call()


def test_tiled_signatures_mirror_the_one_workgroup_calls():
    from neural_astar import ops
    from neural_astar.planner import NeuralAstar, VanillaAstar
    from neural_astar.planner.differentiable_astar import DifferentiableAstar
    assert list(inspect.signature(ops.shortest_paths_tiled).parameters) == list(inspect.signature(ops.shortest_paths).parameters)
    sig = inspect.signature(ops.shortest_paths_tiled)
    assert sig.parameters["lambda_"].default is None and sig.parameters["min_cost"].default == 2.0 ** -10 and sig.parameters["neighbor_mask"].default is None
    assert inspect.signature(ops.path_masks_tiled).parameters["max_rounds"].default is None
    assert inspect.signature(ops.path_masks_tiled_backward).parameters["max_rounds"].default is None
    for cls in (DifferentiableAstar, VanillaAstar, NeuralAstar):
        assert list(inspect.signature(cls.shortest_paths_tiled).parameters) == list(inspect.signature(cls.shortest_paths).parameters)
    assert "BLOCKS" in ops.shortest_paths_tiled.__doc__ and "NOT a tuned number" in ops.shortest_paths_tiled.__doc__


# ---- 4: one definition ------------------------------------------------------------------------------------------------------------------------------------
def test_the_definition_is_the_one_workgroup_calls_and_takes_maps_above_its_limit():
    """tests/path_masks_oracle.py is the definition of BOTH headers: its status codes are the library's, and nothing in it knows a map size --
    an open 129x128 map (16512 cells, above the one-workgroup limit) goes through it like any other map"""
    from neural_astar import _native
    assert (PO.STATUS_BAD_SHAPE, PO.STATUS_UNSOLVABLE, PO.STATUS_BAD_COST, PO.STATUS_PLATEAU) == (
        _native.NASTAR_ERR_BAD_SHAPE, _native.NASTAR_ERR_UNSOLVABLE, _native.NASTAR_ERR_BAD_COST, _native.NASTAR_ERR_PLATEAU)
    f32 = np.float32
    H, W = 129, 128
    cost, passable, goal = np.ones((H, W), f32), np.ones((H, W), f32), np.zeros((H, W), f32)
    goal[64, 40] = 1
    n0 = 64 * W
    got = PO.path(cost, goal, passable, n0)                                 # along the row: "right" is the first action among the equals
    assert got.status == 0 and got.cost == 40 and got.cells == list(range(n0, n0 + 41))
    g = np.zeros((H, W), f32)
    g[64, 1:40] = 1                                                         # push the route off that row
    w = PO.perturbed(cost, g, 20.0, 2.0 ** -10)
    assert w[64, 1] == 21 and w[63, 1] == 1
    grad, st, fwd, lam = PO.backward(cost, goal, passable, n0, g, 20.0, 2.0 ** -10)
    assert st == 0 and lam.cost == 40 and not np.array_equal(lam.mask, fwd.mask) and set(np.unique(grad).tolist()) == {-0.05000000074505806, 0.0, 0.05000000074505806}
