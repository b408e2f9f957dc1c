"""CPU: the tiled entropy-regularised cost-to-go field and its checkpointed gradient (include/nastar_soft_fields_tiled.h,
``ops.soft_cost_to_go_tiled``) -- everything that needs no GPU.

1. the fourteenth header against ``_native.SOFT_FIELD_TILED_SIGNATURES``; the thirteenth and its table are what they were;
2. the library exports every symbol; abi, limit and tile; ``tape_bytes`` and the workspace sizes;
3. every refusal the entry points make before any HIP call, and their order;
4. the Python refusals made before a launch, and the planner methods;
5. the float32 restatement of the definition, on the cases the GPU tests compare with float64, stays below a quarter of the bounds.
"""
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch

import soft_fields_oracle as SO
import soft_fields_tiled_cases as TC
from test_fields import _defines, _prototypes

f32, f64 = np.float32, np.float64
NAMES = ["nastar_soft_cost_to_go_tiled", "nastar_soft_cost_to_go_tiled_with_sweeps", "nastar_soft_fields_backward_tiled", "nastar_soft_fields_tile",
         "nastar_soft_fields_tiled_abi", "nastar_soft_fields_tiled_backward_workspace_bytes", "nastar_soft_fields_tiled_max_cells",
         "nastar_soft_fields_tiled_tape_bytes", "nastar_soft_fields_tiled_workspace_bytes"]
FWD_ARGS = ["cost", "goal", "passable", "B", "H", "W", "neighbor_mask", "tau", "horizon", "dist_out", "policy_out", "status_out", "tape", "tape_bytes",
            "checkpoint_every", "workspace", "workspace_bytes"]
SIZE_MAX = 2 ** 64 - 1


# ---- 1, 2: header, binding, library ---------------------------------------------------------------------------------------------------------------
def test_fourteenth_header_and_tiled_soft_field_signatures_agree():
    from neural_astar import _native
    protos = _prototypes("nastar_soft_fields_tiled.h")
    assert sorted(protos) == sorted(_native.SOFT_FIELD_TILED_SIGNATURES) == NAMES
    for name, (ret, args) in protos.items():
        assert _native.SOFT_FIELD_TILED_SIGNATURES[name] == ret + " " + "".join(k for k, _ in args), name
    assert [n for _, n in protos["nastar_soft_cost_to_go_tiled"][1]] == FWD_ARGS + ["stream"]
    assert [n for _, n in protos["nastar_soft_cost_to_go_tiled_with_sweeps"][1]] == FWD_ARGS + ["sweeps_per_launch", "stream"]
    assert [n for _, n in protos["nastar_soft_fields_backward_tiled"][1]] == [
        "cost", "goal", "passable", "tape", "tape_bytes", "checkpoint_every", "grad_dist", "B", "H", "W", "neighbor_mask", "tau", "horizon",
        "grad_cost_out", "status_out", "workspace", "workspace_bytes", "stream"]
    # a table of its own; the thirteenth header, its table and nastar.h are what they were
    for table in (_native.SIGNATURES, _native.FIELD_SIGNATURES, _native.TILED_FIELD_SIGNATURES, _native.SOFT_FIELD_SIGNATURES):
        assert not set(_native.SOFT_FIELD_TILED_SIGNATURES) & set(table)
    assert len(_native.SOFT_FIELD_SIGNATURES) == 6 == len(_prototypes("nastar_soft_fields.h")) and len(_native.SIGNATURES) == 74
    assert _defines("nastar_soft_fields_tiled.h") == {"NASTAR_SOFT_FIELDS_TILED_ABI": 1}      # no new code, no new version
    assert _defines("nastar_soft_fields.h") == {"NASTAR_SOFT_FIELDS_ABI": 1} and _defines("nastar.h")["NASTAR_VERSION"] == 800


def _tile(lib):
    th, tw, S = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    assert lib.nastar_soft_fields_tile(ctypes.addressof(th), ctypes.addressof(tw), ctypes.addressof(S)) == 0
    return th.value, tw.value, S.value


def test_library_exports_the_tiled_soft_field_symbols():
    from neural_astar import _native, ops
    lib = _native.load()
    for sym in _native.SOFT_FIELD_TILED_SIGNATURES:
        assert hasattr(lib, sym), sym
    assert lib.nastar_soft_fields_tiled_abi() == 1
    assert lib.nastar_soft_fields_tiled_max_cells() == ops.SOFT_FIELDS_TILED_MAX_CELLS == 1179648 == 1024 * 1152
    th, tw, S = _tile(lib)
    # the bit-equality tests need maps with seams in both directions inside the one-workgroup limits
    assert th >= 1 and tw >= 1 and S >= 1
    assert (th + 3) * (tw + 5) <= ops.SOFT_FIELDS_GRAD_MAX_CELLS and (2 * th + 1) * (tw + 1) <= ops.SOFT_FIELDS_MAX_CELLS
    assert lib.nastar_soft_fields_tile(None, None, None) == 0
    assert len(lib.nastar_soft_cost_to_go_tiled.argtypes) == 18 == len(lib.nastar_soft_fields_backward_tiled.argtypes)
    assert len(lib.nastar_soft_cost_to_go_tiled_with_sweeps.argtypes) == 19
    assert {"soft_cost_to_go_tiled", "maxent_path_nll_tiled", "soft_fields_tiled_forward", "soft_fields_tiled_backward",
            "SOFT_FIELDS_TILED_MAX_CELLS"} <= set(ops.__all__)


def test_tape_and_workspace_bytes():
    from neural_astar import _native
    lib = _native.load()
    tape, bws, fws = (lib.nastar_soft_fields_tiled_tape_bytes, lib.nastar_soft_fields_tiled_backward_workspace_bytes,
                      lib.nastar_soft_fields_tiled_workspace_bytes)
    big = 2 ** 31 - 1
    for size, strict, c_big in ((tape, True, 1), (bws, False, big)):
        assert [size(0, 4, 4, 4, 2), size(4, 0, 4, 4, 2), size(4, 4, -1, 4, 2), size(4, 4, 4, 0, 2), size(4, 4, 4, 4, 0), size(4, 4, 4, 4, -7)] == [0] * 6
        assert size(big, 1024, 1152, big, c_big) == SIZE_MAX   # does not fit: nothing is that large
        # monotone in B and in the horizon (the tape strictly: a map more is a plane more, c sweeps more are a checkpoint more)
        for B, H, W, K, c in [(1, 1, 1, 1, 1), (2, 32, 33, 130, 12), (4096, 64, 64, 64, 8), (1, 1024, 1024, 4096, 64), (3, 67, 69, 97, 1)]:
            assert 0 < size(B, H, W, K, c) <= size(B + 1, H, W, K, c), (B, H, W, K, c)
            assert size(B, H, W, K, c) <= size(B, H, W, K + 1, c) <= size(B, H, W, K + c, c), (B, H, W, K, c)
            if strict:
                assert size(B, H, W, K, c) < size(B + 1, H, W, K, c) and size(B, H, W, K, c) < size(B, H, W, K + c, c), (B, H, W, K, c)
    assert bws(2, 32, 33, 130, 12) < bws(3, 32, 33, 130, 12) and bws(2, 32, 33, 5, 12) < bws(2, 32, 33, 6, 12)
    assert [fws(0, 4, 4), fws(4, 0, 4), fws(4, 4, -1)] == [0, 0, 0] and fws(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1) == SIZE_MAX
    assert 0 < fws(1, 64, 64) < fws(2, 64, 64) < fws(2, 64, 65)
    for B, H, W, K in [(1, 1, 1, 1), (3, 5, 7, 24), (2, 67, 69, 97), (1, 1024, 1024, 4096), (1, 1024, 1152, 8)]:
        plane = B * H * W * 4
        assert tape(B, H, W, K, 1) >= B * K * H * W * 4        # c = 1: every plane
        assert tape(B, H, W, K, K + 5) == plane                # nothing but plane K
        c = math.isqrt(K - 1) + 1 if K > 1 else 1              # ceil(sqrt(K)), the Python default
        assert (c - 1) ** 2 < K <= c * c
        # the checkpoints and plane K: at most K / c + 2 planes; with the segment buffer of the backward, at most K / c + c + 2 ...
        assert tape(B, H, W, K, c) <= (K // c + 2) * plane
        fixed = bws(B, H, W, K, c) - (min(c, K) - 1) * plane
        assert tape(B, H, W, K, c) + (bws(B, H, W, K, c) - fixed) <= (K // c + c + 2) * plane
        # ... and what else the backward keeps depends neither on the horizon nor on c: six planes' worth, the flags and padding
        assert fixed == bws(B, H, W, 1, 1) == bws(B, H, W, 3 * K + 1, 2) - plane and 6 * plane <= fixed <= 6 * plane + 8 * B + 6 * 16 + 256
    # one 1024 x 1024 map at the default horizon: about 0.5 GiB with the default spacing where every plane is 16 GiB
    assert tape(1, 1024, 1024, 4096, 1) >= 16 * 2 ** 30
    assert tape(1, 1024, 1024, 4096, 64) + bws(1, 1024, 1024, 4096, 64) <= 0.6 * 2 ** 30


# ---- 3: refusals, made before any HIP call -----------------------------------------------------------------------------------------------------------
P = 0x10000  # never dereferenced: every call below is refused on its arguments
BIG = 1 << 40


def _fwd(**over):
    a = dict(cost=P, goal=P, passable=P, B=2, H=8, W=8, neighbor_mask=0x1EF, tau=0.5, horizon=16, dist_out=P, policy_out=None, status_out=P,
             tape=None, tape_bytes=0, checkpoint_every=4, workspace=P, workspace_bytes=BIG, stream=None)
    a.update(over)
    return a


def _bwd(**over):
    a = dict(cost=P, goal=P, passable=P, tape=P, tape_bytes=2 * 64 * 5 * 4, checkpoint_every=4, grad_dist=P, B=2, H=8, W=8, neighbor_mask=0x1EF,
             tau=0.5, horizon=16, grad_cost_out=P, status_out=P, workspace=P, workspace_bytes=BIG, stream=None)
    a.update(over)
    return a


SHARED = [(dict(neighbor_mask=0x1FF), 2), (dict(neighbor_mask=0x200), 2), (dict(cost=None), 5), (dict(goal=None), 5), (dict(passable=None), 5),
          (dict(status_out=None), 5), (dict(workspace=None), 5), (dict(B=0), 1), (dict(H=0), 1), (dict(W=-1), 1), (dict(horizon=0), 1),
          (dict(horizon=-3), 1), (dict(checkpoint_every=0), 1), (dict(checkpoint_every=-2), 1),
          (dict(tau=0.0), 1), (dict(tau=-1.0), 1), (dict(tau=float("nan")), 1), (dict(tau=float("inf")), 1),
          (dict(neighbor_mask=0x010, cost=None), 2),                 # the mask is looked at first
          (dict(cost=None, B=0), 5), (dict(workspace=None, checkpoint_every=0), 5),   # a NULL before the shape
          (dict(tau=0.0, H=1024, W=1153), 1), (dict(checkpoint_every=0, H=1024, W=1153), 1),   # the shape, tau and c before the limit
          (dict(H=1024, W=1153), 2), (dict(H=1, W=1179649), 2), (dict(H=65536, W=65536), 2),
          (dict(B=(1 << 24) + 1, H=1, W=1), 2),                      # more than 2^24 tiles in the batch
          (dict(H=1024, W=1153, workspace_bytes=0), 2),              # the limit before the workspace
          (dict(workspace_bytes=0), 6), (dict(workspace=P + 8), 6)]


def _ws_bytes(lib, backward, a):
    if backward:
        return lib.nastar_soft_fields_tiled_backward_workspace_bytes(a["B"], a["H"], a["W"], a["horizon"], a["checkpoint_every"])
    return lib.nastar_soft_fields_tiled_workspace_bytes(a["B"], a["H"], a["W"])


@pytest.mark.parametrize("over,rc", SHARED + [
    (dict(dist_out=None), 5), (dict(tape=P, tape_bytes=2 * 64 * 5 * 4 - 1), 6), (dict(tape=P + 4, tape_bytes=BIG), 6), (dict(tape=P, tape_bytes=0), 6),
    (dict(H=1024, W=1153, tape=P, tape_bytes=0), 2),               # the limit before the tape
    (dict(tape=P, tape_bytes=0, workspace_bytes=0), 6)])
def test_soft_cost_to_go_tiled_refuses_bad_arguments_without_a_device(over, rc):
    from neural_astar import _native
    lib = _native.load()
    S = _tile(lib)[2]
    assert lib.nastar_soft_cost_to_go_tiled(*_fwd(**over).values()) == rc
    assert lib.nastar_soft_cost_to_go_tiled(*_fwd(**dict(dict(policy_out=P), **over)).values()) == rc
    for sweeps in (1, S):
        a = list(_fwd(**over).values())
        assert lib.nastar_soft_cost_to_go_tiled_with_sweeps(*a[:-1], sweeps, a[-1]) == rc
    assert lib.nastar_last_error() == b""


def test_sweeps_per_launch_and_the_exact_workspace_size_are_checked_without_a_device():
    from neural_astar import _native
    lib = _native.load()
    S = _tile(lib)[2]
    a = list(_fwd().values())
    for sweeps, rc in ((0, 1), (-1, 1), (S + 1, 1)):
        assert lib.nastar_soft_cost_to_go_tiled_with_sweeps(*a[:-1], sweeps, a[-1]) == rc
    bad_mask = list(_fwd(neighbor_mask=0x1FF).values())
    assert lib.nastar_soft_cost_to_go_tiled_with_sweeps(*bad_mask[:-1], 0, bad_mask[-1]) == 2          # the mask first
    too_big = list(_fwd(H=1024, W=1153).values())
    assert lib.nastar_soft_cost_to_go_tiled_with_sweeps(*too_big[:-1], S + 1, too_big[-1]) == 1        # the shape before the limit
    # one byte short of what the size functions say is refused
    need = _ws_bytes(lib, False, _fwd())
    assert need > 0 and lib.nastar_soft_cost_to_go_tiled(*_fwd(workspace_bytes=need - 1).values()) == 6
    need = _ws_bytes(lib, True, _bwd())
    assert need > 0 and lib.nastar_soft_fields_backward_tiled(*_bwd(workspace_bytes=need - 1).values()) == 6
    assert lib.nastar_last_error() == b""


@pytest.mark.parametrize("over,rc", SHARED + [
    (dict(tape=None), 5), (dict(grad_dist=None), 5), (dict(grad_cost_out=None), 5),
    (dict(H=1024, W=1153, tape_bytes=0), 2),                       # the limit before the tape
    (dict(tape_bytes=2 * 64 * 5 * 4 - 1), 6), (dict(tape=P + 8), 6), (dict(horizon=20), 6), (dict(B=3), 6),
    (dict(checkpoint_every=3), 6),                                 # 16 / 3 + 1 = 6 planes: the tape of another spacing is too small
    (dict(tape_bytes=0, workspace_bytes=0), 6)])
def test_soft_fields_backward_tiled_refuses_bad_arguments_without_a_device(over, rc):
    from neural_astar import _native
    lib = _native.load()
    assert lib.nastar_soft_fields_backward_tiled(*_bwd(**over).values()) == rc
    assert lib.nastar_last_error() == b""


# ---- 4: Python refusals before a launch; the planner methods ----------------------------------------------------------------------------------------
def test_refusals_before_a_launch_and_the_planner_methods():
    from neural_astar import ops
    from neural_astar.planner import NeuralAstar, VanillaAstar
    from neural_astar.planner.differentiable_astar import DifferentiableAstar
    assert list(inspect.signature(ops.soft_cost_to_go_tiled).parameters) == ["cost_maps", "goal_maps", "obstacles_maps", "tau", "horizon",
                                                                             "neighbor_mask", "policies", "differentiable", "checkpoint_every"]
    assert list(inspect.signature(ops.maxent_path_nll_tiled).parameters) == list(inspect.signature(ops.maxent_path_nll).parameters) + ["checkpoint_every"]
    for cls in (DifferentiableAstar, VanillaAstar, NeuralAstar):
        prm = inspect.signature(cls.soft_cost_to_go_tiled).parameters
        assert prm["differentiable"].default is False and prm["policies"].default is False and prm["horizon"].default is None, cls
        assert prm["checkpoint_every"].default is None, cls
        prm = inspect.signature(cls.maxent_path_nll).parameters
        assert prm["tiled"].default is False and prm["checkpoint_every"].default is None and prm["horizon"].default is None, cls
    m = torch.ones(2, 1, 8, 8, requires_grad=True)
    for c in (0, -1, 1.5, True, "3", 2 ** 31):
        with pytest.raises(ValueError, match="checkpoint_every"):
            ops.soft_cost_to_go_tiled(m, m, m, 0.5, checkpoint_every=c)
        with pytest.raises(ValueError, match="checkpoint_every"):
            ops.maxent_path_nll_tiled(m, m, m, m, m, 0.5, checkpoint_every=c)
        with pytest.raises(ValueError, match="checkpoint_every"):
            ops.soft_fields_tiled_backward(m, m, m, torch.zeros(8, dtype=torch.uint8), m, 0.5, checkpoint_every=c)
        with pytest.raises(ValueError, match="checkpoint_every"):
            DifferentiableAstar().maxent_path_nll(m, m, m, m, m, 0.5, tiled=True, checkpoint_every=c)
    with pytest.raises(ValueError, match="checkpoint_every"):      # the one-workgroup field has no checkpoints
        DifferentiableAstar().maxent_path_nll(m, m, m, m, m, 0.5, checkpoint_every=4)
    assert [ops._checked_checkpoint_every(None, K) for K in (1, 2, 4, 5, 97, 356, 4096, 4097)] == [1, 2, 2, 3, 10, 19, 64, 65]
    for tau in (0.0, -0.5, float("nan"), float("inf"), True, None):
        with pytest.raises(ValueError, match="tau"):
            ops.soft_cost_to_go_tiled(m, m, m, tau)
    for horizon in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="horizon"):
            ops.soft_cost_to_go_tiled(m, m, m, 0.5, horizon=horizon)
    with pytest.raises(ValueError, match="sweeps_per_launch"):
        ops.soft_fields_tiled_forward(m, m, m, 0.5, sweeps_per_launch=0)
    with pytest.raises(ValueError, match="neighbor_mask"):
        ops.soft_cost_to_go_tiled(m, m, m, 0.5, neighbor_mask=0x1FF)
    with pytest.raises(ValueError, match="share one"):
        ops.soft_cost_to_go_tiled(m, torch.ones(2, 1, 8, 9), m, 0.5)
    # tensors on the CPU: there is no CPU path
    for diff in (False, True):
        with pytest.raises(RuntimeError, match="HIP device"):
            ops.soft_cost_to_go_tiled(m, m, m, 0.5, differentiable=diff)
    big = torch.ones(1, 1, 96, 136)                               # above both one-workgroup limits: taken (and refused for the device only)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.soft_cost_to_go_tiled(big, big, big, 0.5, differentiable=True)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.maxent_path_nll_tiled(big, big, big, big, big, 0.5)
    with pytest.raises(NotImplementedError, match="12288"):       # the one-workgroup calls refuse it as they did
        ops.soft_cost_to_go(big, big, big, 0.5)
    with pytest.raises(NotImplementedError, match="6144"):
        ops.maxent_path_nll(big, big, big, big, big, 0.5)
    with pytest.raises(NotImplementedError, match="6144"):
        DifferentiableAstar().maxent_path_nll(big, big, big, big, big, 0.5)
    assert ops.SOFT_FIELDS_TILED_MAX_CELLS == 1179648
    ok = torch.ones(1, 1024, 1152)                                # the limit itself is taken
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.soft_cost_to_go_tiled(ok, ok, ok, 0.5, horizon=2)
    huge = torch.ones(1, 1, 1179649)                              # one cell more
    with pytest.raises(NotImplementedError, match="1179648"):
        ops.soft_cost_to_go_tiled(huge, huge, huge, 0.5)
    with pytest.raises(NotImplementedError, match="1179648"):
        ops.soft_fields_tiled_forward(huge, huge, huge, 0.5)
    with pytest.raises(NotImplementedError, match="1179648"):
        ops.soft_fields_tiled_backward(huge, huge, huge, torch.zeros(8, dtype=torch.uint8), huge, 0.5)
    with pytest.raises(NotImplementedError, match="1179648"):
        VanillaAstar().soft_cost_to_go_tiled(huge, huge, 0.5)
    with pytest.raises(ValueError, match="tau"):
        NeuralAstar().maxent_path_nll(m, m, m, m, -1.0, tiled=True)
    with pytest.raises(RuntimeError, match="HIP device"):
        DifferentiableAstar().soft_cost_to_go_tiled(m, m, m, 0.5)


# ---- 5: the float32 restatement on the cases of the GPU tests ---------------------------------------------------------------------------------------
def _restatement(cost, passable, goal, G, tau, K, mask):
    """(forward, backward) error of the float32 restatement against float64, relative as SO.rel_err is"""
    a, _, _ = SO.soft_fields(cost, goal, passable, tau, K, mask)
    b, _, _ = SO.soft_fields(cost, goal, passable, tau, K, mask, f32)
    assert np.array_equal(np.isfinite(a), np.isfinite(b))
    ga = SO.soft_field_grads(cost, goal, passable, G, tau, K, mask)[0]
    gb = SO.soft_field_grads(cost, goal, passable, G, tau, K, mask, f32)[0]
    return SO.rel_err(b, a), SO.rel_err(gb, ga)


@pytest.mark.parametrize("H,W,B,seed,K", TC.ABOVE, ids=lambda v: str(v))
def test_float32_restatement_of_the_cases_above_the_old_limits_stays_below_a_quarter_of_the_bounds(H, W, B, seed, K):
    """measured with this file's upstream gradients (forward / backward): 48x130 K=60 2.2e-7 .. 3.1e-7 / 2.9e-7 .. 2.9e-6; 130x140 K=97
    2.9e-7 .. 4.7e-7 / 2.3e-6 .. 7.1e-6; a quarter of the bounds is 5.33e-7 / 1.7e-5"""
    cost, passable, goal = TC.maps(H, W, B, seed)
    for mask in TC.ABOVE_MASKS:
        for tau in SO.TAUS:
            live = (passable != 0) & (goal == 0) & np.isfinite(SO.soft_fields(cost, goal, passable, tau, K, mask)[0])
            fwd, bwd = _restatement(cost, passable, goal, TC.upstream(seed, live), tau, K, mask)
            print(f"{H}x{W} K={K} tau={tau} mask={mask:#05x}: float32 restatement forward {fwd:.3e}, backward {bwd:.3e}")
            assert 0 < fwd <= SO.FWD_RTOL / 4 and 0 < bwd <= SO.BWD_RTOL / 4


@pytest.mark.parametrize("tau", TC.MAXENT_TAUS)
def test_float32_restatement_of_the_maxent_case_stays_below_a_quarter_of_the_bounds(tau):
    cost, passable, goal, start = TC.maxent_maps()
    fwd, bwd = _restatement(cost, passable, goal, (start != 0).astype(f64), tau, TC.ABOVE[1][4], SO.MOORE8)
    print(f"maxent tau={tau}: float32 restatement forward {fwd:.3e}, backward (expected visits) {bwd:.3e}")
    assert 0 < fwd <= SO.FWD_RTOL / 4 and 0 < bwd <= SO.BWD_RTOL / 4


def test_float32_restatement_of_the_far_corner_stays_below_a_quarter_of_the_bounds():
    cost, passable, goal = (TC.corner_window(a) for a in TC.corner_maps())
    G = TC.corner_window(TC.corner_upstream())
    gy, gx = np.argwhere(goal[0] != 0)[0]
    sy, sx = np.argwhere(G[0] != 0)[0]
    # the window holds everything within K moves of the goal, and its cut edges are more than K cells away
    assert gy == goal.shape[1] - 1 and min(gy, gx) > TC.CORNER_K and max(abs(gy - sy), abs(gx - sx)) == 2
    hops = SO.hops(goal[0], passable[0])
    assert hops[sy, sx] == 2
    for edge in (hops[0], hops[:, 0]):
        assert ((edge < 0) | (edge > TC.CORNER_K)).all()
    fwd, bwd = _restatement(cost, passable, goal, G, TC.CORNER_TAU, TC.CORNER_K, SO.MOORE8)
    print(f"far corner K={TC.CORNER_K}: float32 restatement forward {fwd:.3e}, backward {bwd:.3e}")
    assert 0 < fwd <= SO.FWD_RTOL / 4 and 0 < bwd <= SO.BWD_RTOL / 4
