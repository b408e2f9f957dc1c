"""CPU: the gradient of the cost-to-go field for maps of up to 1024x1152 (include/nastar_fields_grad_tiled.h, ``ops.fields_backward_tiled``,
``ops.cost_to_go_tiled(..., differentiable=True)``) -- everything that needs no GPU.

1. the scheme (tests/fields_grad_tiled_oracle.py: random tile order, every halo word fresh or one round stale) equals the untiled in-order
   evaluation bit for bit, ends within H*W + 1 rounds, equals ``fields_grad_oracle`` exactly for integer-valued G and within 6g's tolerance
   for float G; marking nobody -- the bug -- is seen; too few rounds give status 10 and zeros; a plateau gives 11 and zeros;
2. the ninth header against ``_native.FIELD_GRAD_TILED_SIGNATURES``; the library's symbols, abi, limit and workspace size;
3. every refusal the two status-returning entry points make before any HIP call, and their order;
4. the Python refusals made without a device, and the new keyword on ``ops.cost_to_go_tiled`` and the planners' ``cost_to_go_tiled``.
"""
import functools
import inspect

import numpy as np
import pytest
import torch

import fields_grad_oracle as GO
import fields_grad_tiled_oracle as GT
import fields_oracle as FO
import fields_tiled_oracle as TO
import heuristic_oracle as HO
from test_fields import _defines, _prototypes

f32, f64 = np.float32, np.float64
DIRECTED = 0x0EB
SHAPES = [(33, 47, (16, 16)), (65, 65, (64, 64)), (70, 130, (64, 64)), (130, 259, (64, 64))]


@functools.lru_cache(maxsize=None)
def _case(H, W, mask):
    """cost U(0.5, 1.5), about 30 % obstacles, one goal on a passable cell, the field, an integer-valued and a float upstream gradient"""
    rng = np.random.default_rng([H, W, mask])
    passable = (rng.random((H, W)) > 0.3).astype(f32)
    goal = np.zeros((H, W), f32)
    gy, gx = int(rng.integers(H)), int(rng.integers(W))
    goal[gy, gx] = passable[gy, gx] = 1
    cost = (0.5 + rng.random((H, W))).astype(f32)
    dist, _, status = FO.field(cost, goal, passable, mask)
    assert status == 0
    Gi = rng.integers(-8, 9, (H, W)).astype(f32)
    Gf = rng.standard_normal((H, W)).astype(f32)
    for a in (cost, goal, passable, dist, Gi, Gf):
        a.setflags(write=False)
    return cost, goal, passable, dist, Gi, Gf


# ---- 1: the scheme ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", [HO.MOORE8, HO.VON_NEUMANN, DIRECTED])
@pytest.mark.parametrize("H,W,tile", SHAPES)
def test_tiled_scheme_is_the_in_order_evaluation(H, W, tile, mask):
    cost, goal, passable, dist, Gi, Gf = _case(H, W, mask)
    ref = GO.field_grad(cost, goal, passable, Gf, mask)
    assert ref.status == 0 and np.array_equal(ref.dist, dist) and ref.live.sum() > 20
    F = GT.forest(dist, goal, passable, mask)                       # the forest from dist alone is the definition's
    assert not F.plateau and np.array_equal(F.live, ref.live) and np.array_equal(F.succ.reshape(H, W), ref.succ)
    want, want32, st = GT.in_order(dist, goal, passable, Gf, mask)
    assert st == 0
    for seed in range(3):                                           # random tile order, random fresh / stale halo words
        A, grad, st, rounds, visits = GT.tiled_grad(dist, goal, passable, Gf, mask, tile, np.random.default_rng([seed, H, W]))
        assert st == 0 and A.tobytes() == want.tobytes() and grad.tobytes() == want32.tobytes(), seed
        assert 1 <= rounds <= H * W + 1 and visits >= rounds
    A, grad, st, rounds2, _ = GT.tiled_grad(dist, goal, passable, Gf, mask, tile)       # every halo fresh, tiles in index order
    assert st == 0 and A.tobytes() == want.tobytes()
    print(f"{H}x{W} {hex(mask)}: {rounds} rounds, {visits} tile visits with random halos; {rounds2} rounds with fresh ones")
    # float G: the definition adds in another order -- 6g's derived tolerance, 2^-23 |ref| + 1e-9 sum|G|
    tol = 2.0 ** -23 * np.abs(ref.A) + 1e-9 * np.abs(Gf[ref.live].astype(f64)).sum()
    assert (np.abs(want - ref.A) <= tol)[ref.live].all() and not grad[~ref.live].any()
    # integer-valued G: every order is exact
    Ai, gi, st, _, _ = GT.tiled_grad(dist, goal, passable, Gi, mask, tile, np.random.default_rng(7))
    refi = GO.field_grad(cost, goal, passable, Gi, mask)
    assert st == 0 and np.array_equal(Ai, refi.A) and np.array_equal(gi, refi.grad) and np.array_equal(Ai, np.round(Ai))
    assert np.array_equal(GT.in_order(dist, goal, passable, Gi, mask)[0], refi.A)


@pytest.mark.parametrize("mask", [HO.MOORE8, HO.VON_NEUMANN])
@pytest.mark.parametrize("H,W,tile", [(33, 47, (16, 16)), (70, 130, (64, 64))])
def test_tiled_scheme_on_a_serpentine(H, W, tile, mask):
    cost, goal, passable, walls = TO.serpentine(H, W)
    dist, _, _ = FO.field(cost, goal, passable, mask)
    G = np.random.default_rng(H).standard_normal((H, W)).astype(f32)
    want, want32, st = GT.in_order(dist, goal, passable, G, mask)
    assert st == 0
    for seed in range(2):
        A, grad, st, rounds, _ = GT.tiled_grad(dist, goal, passable, G, mask, tile, np.random.default_rng([seed, H]))
        assert st == 0 and A.tobytes() == want.tobytes() and grad.tobytes() == want32.tobytes()
        assert walls // 2 <= rounds <= H * W + 1                    # the chain crosses tile borders again and again
    ones = np.ones((H, W), f32)                                     # G = 1: subtree sizes, exact integers
    sizes, _, _, _, _ = GT.tiled_grad(dist, goal, passable, ones, mask, tile, np.random.default_rng(3))
    ref = GO.field_grad(cost, goal, passable, ones, mask)
    assert np.array_equal(sizes, ref.A) and sizes.max() > walls * (W - 2)


def test_marking_nobody_is_seen_and_too_few_rounds_give_zeros():
    H, W, tile = 70, 130, (64, 64)
    cost, goal, passable, walls = TO.serpentine(H, W)
    dist, _, _ = FO.field(cost, goal, passable, HO.VON_NEUMANN)
    ones = np.ones((H, W), f32)
    want, _, _ = GT.in_order(dist, goal, passable, ones, HO.VON_NEUMANN)
    bad, _, st, rounds, _ = GT.tiled_grad(dist, goal, passable, ones, HO.VON_NEUMANN, tile, np.random.default_rng(0), mark="none")
    assert st == 0 and rounds == 1 and not np.array_equal(bad, want)        # the bug the directed-mask tests look for
    A, grad, st, rounds, _ = GT.tiled_grad(dist, goal, passable, ones, HO.VON_NEUMANN, tile, np.random.default_rng(0), max_rounds=2)
    assert st == GT.STATUS_NO_CONVERGENCE == 10 and rounds == 2 and not A.any() and not grad.any()   # a partial sum is a bound of nothing


def test_plateau_and_no_goal():
    cost, goal, passable, dist, Gi, Gf = (np.array(a) for a in _case(33, 47, HO.MOORE8))
    gy, gx = np.argwhere(goal != 0)[0]
    xs = slice(max(0, gx - 3), min(47, gx + 4))
    cost[gy, xs], passable[gy, xs] = 0, 1
    d, _, _ = FO.field(cost, goal, passable)
    assert GT.forest(d, goal, passable).plateau and GO.field_grad(cost, goal, passable, Gf).status == 11
    A, grad, st, rounds, visits = GT.tiled_grad(d, goal, passable, Gf, tile=(16, 16))
    assert st == GT.STATUS_PLATEAU == 11 and not A.any() and not grad.any() and rounds == 0
    assert GT.in_order(d, goal, passable, Gf)[2] == 11
    none = np.zeros_like(goal)
    d, _, _ = FO.field(cost, none, passable)
    A, grad, st, rounds, _ = GT.tiled_grad(d, none, passable, Gf, tile=(16, 16))
    assert st == 0 and rounds == 0 and not grad.any()               # no goal: nothing is live, NASTAR_OK


def test_what_is_not_live_is_never_read():
    cost, goal, passable, dist, Gi, Gf = _case(65, 65, HO.MOORE8)
    F = GT.forest(dist, goal, passable)
    G = np.where(F.live, Gf, f32(np.nan))
    assert np.isnan(G).sum() > 10
    A, grad, st, _, _ = GT.tiled_grad(dist, goal, passable, G, rng=np.random.default_rng(1))
    want, want32, _ = GT.in_order(dist, goal, passable, Gf)
    assert st == 0 and A.tobytes() == want.tobytes() and np.isfinite(grad).all()


# ---- 1b: an upstream gradient that SHOWS the order of the children ------------------------------------------------------------------------------------
ORDER_CASES = [(H, W, mask) for H, W in ((20, 45), (70, 130)) for mask in (HO.MOORE8, DIRECTED)]


@functools.lru_cache(maxsize=None)
def _order_case(H, W, mask):
    """two maps [2,H,W]: cost U(0.5, 1.5), about 20 % obstacles, one goal on a passable cell, the field, and G drawn per cell from
    {+2^60, -2^60, 1.0}.  A Gaussian G hides the order of an fp64 sum behind the fp32 rounding of the result; here 2^60 + 1 absorbs the 1
    (the ulp of 2^60 in binary64 is 256) and 2^60 - 2^60 + 1 keeps it, so the order of the children reaches the fp32 output.  Shared with
    the GPU pin (tests/test_fields_grad_tiled_gpu.py), never modified."""
    rng = np.random.default_rng([H, W, mask, 1])
    passable = (rng.random((2, H, W)) > 0.2).astype(f32)
    goal = np.zeros((2, H, W), f32)
    for b in range(2):
        gy, gx = int(rng.integers(H)), int(rng.integers(W))
        goal[b, gy, gx] = passable[b, gy, gx] = 1
    cost = (0.5 + rng.random((2, H, W))).astype(f32)
    G = rng.choice(np.array([2.0 ** 60, -2.0 ** 60, 1.0], f32), size=(2, H, W))
    fields = [FO.field(cost[b], goal[b], passable[b], mask) for b in range(2)]
    assert [st for _, _, st in fields] == [0, 0]
    dist = np.stack([d for d, _, _ in fields])
    want = [GT.in_order(dist[b], goal[b], passable[b], G[b], mask) for b in range(2)]
    assert [st for _, _, st in want] == [0, 0]
    grad = np.stack([g32 for _, g32, _ in want])
    for a in (goal, passable, dist, G, grad):
        a.setflags(write=False)
    return goal, passable, dist, G, grad


def _children_reversed(dist, goal, passable, G, mask):
    """``GT.in_order`` with one change: every cell adds its children in the REVERSED order"""
    F = GT.forest(dist, goal, passable, mask)
    H, W = F.live.shape
    assert not F.plateau
    g = np.asarray(G, f32).reshape(-1).astype(np.float64).tolist()
    A = [0.0] * (H * W)
    for n in F.order.tolist():
        v = g[n]
        for c in reversed(F.kids[n]):
            v += A[c]
        A[n] = v
    A = np.array(A).reshape(H, W)
    return np.where(F.live, A, 0.0).astype(f32)


@pytest.mark.parametrize("H,W,mask", ORDER_CASES)
def test_the_order_pin_sees_a_reversed_child_order(H, W, mask):
    """what makes tests/test_fields_grad_tiled_gpu.py::test_gradient_bits_are_the_in_order_sum a pin of the ORDER: on its very inputs, adding
    the children the other way round changes fp32 cells of the output"""
    goal, passable, dist, G, grad = _order_case(H, W, mask)
    assert np.isfinite(grad).all()                                  # at most 9100 addends of magnitude 2^60: far below fp32's 2^128
    other = np.stack([_children_reversed(dist[b], goal[b], passable[b], G[b], mask) for b in range(2)])
    assert np.isfinite(other).all()
    changed = [int((other[b].view(np.uint32) != grad[b].view(np.uint32)).sum()) for b in range(2)]
    print(f"{H}x{W} {hex(mask)}: a reversed child order changes {changed} fp32 cells of the two maps")
    assert min(changed) >= 1


# ---- 2: header, binding, library ----------------------------------------------------------------------------------------------------------------------
NAMES =["nastar_fields_backward_tiled", "nastar_fields_backward_tiled_status", "nastar_fields_backward_tiled_workspace_bytes",
         "nastar_fields_grad_tiled_abi", "nastar_fields_grad_tiled_max_cells"]


def test_ninth_header_and_field_grad_tiled_signatures_agree():
    from neural_astar import _native
    protos = _prototypes("nastar_fields_grad_tiled.h")
    assert sorted(protos) == sorted(_native.FIELD_GRAD_TILED_SIGNATURES) == NAMES
    for name, (ret, args) in protos.items():
        assert _native.FIELD_GRAD_TILED_SIGNATURES[name] == ret + " " + "".join(k for k, _ in args), name
    assert [n for _, n in protos["nastar_fields_backward_tiled"][1]] == [
        "dist", "goal", "passable", "grad_dist", "B", "H", "W", "neighbor_mask", "grad_cost_out", "status_out", "visits_out", "workspace",
        "workspace_bytes", "max_rounds", "rounds_out", "stream"]
    assert [n for _, n in protos["nastar_fields_backward_tiled_status"][1]] == [
        "dist", "goal", "passable", "B", "H", "W", "neighbor_mask", "status_out", "workspace", "workspace_bytes", "stream"]
    # a table of its own, and no name that tests/test_capi_library.py counts
    for table in (_native.SIGNATURES, _native.FIELD_SIGNATURES, _native.TILED_FIELD_SIGNATURES, _native.FIELD_GRAD_SIGNATURES):
        assert not set(_native.FIELD_GRAD_TILED_SIGNATURES) & set(table)
    assert not any(n.startswith("nastar_cost_to_go") for n in _native.FIELD_GRAD_TILED_SIGNATURES)
    assert len(_native.SIGNATURES) == 74 and len(_native.FIELD_SIGNATURES) == 4 and len(_native.TILED_FIELD_SIGNATURES) == 6 and len(_native.FIELD_GRAD_SIGNATURES) == 3
    new = _defines("nastar_fields_grad_tiled.h")
    assert new["NASTAR_FIELDS_GRAD_TILED_ABI"] == 1 and "NASTAR_VERSION" not in new and _defines("nastar.h")["NASTAR_VERSION"] == 800
    assert not [k for k in new if k.startswith("NASTAR_ERR_")]      # no new status code: 10 and 11 are the other headers'
    header = open(_header_path()).read()
    assert "BLOCKS" in header and "cannot be captured" in header


def _header_path():
    import os
    return os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nastar_fields_grad_tiled.h")


def test_library_exports_the_field_grad_tiled_symbols():
    from neural_astar import _native, ops
    lib = _native.load()
    for sym in NAMES:
        assert hasattr(lib, sym), sym
    assert lib.nastar_fields_grad_tiled_abi() == 1
    assert lib.nastar_fields_grad_tiled_max_cells() == ops.FIELDS_GRAD_TILED_MAX_CELLS == ops.FIELDS_TILED_MAX_CELLS == lib.nastar_fields_tiled_max_cells() == 1179648
    assert len(lib.nastar_fields_backward_tiled.argtypes) == 16 and len(lib.nastar_fields_backward_tiled_status.argtypes) == 11
    assert {"fields_backward_tiled", "FIELDS_GRAD_TILED_MAX_CELLS", "cost_to_go_tiled"} <= set(ops.__all__)
    ws = lib.nastar_fields_backward_tiled_workspace_bytes
    # 8 B of A and one successor byte per cell, four words per map, two flags per tile -- rounded up to 16
    assert ws(1, 64, 64) == (4096 * 9 + 16 + 8 + 15) // 16 * 16
    assert ws(3, 70, 130) == (3 * 70 * 130 * 9 + 3 * 16 + 3 * 6 * 8 + 15) // 16 * 16
    assert ws(1, 1024, 1152) == (1179648 * 9 + 16 + 288 * 8 + 15) // 16 * 16 and ws(1, 1024, 1152) % 8 == 0
    assert ws(2048, 1024, 1024) == 2048 * (1024 * 1024 * 9 + 16 + 256 * 8)      # B*H*W = 2^31: size_t throughout
    for refused in ((0, 8, 8), (1, 0, 8), (1, 8, -1), (1, 1024, 1153), (1, 65536, 65536), (1 << 23, 70, 130), (-1, 8, 8)):
        assert ws(*refused) == 0, refused


# ---- 3: refusals, made before any HIP call --------------------------------------------------------------------------------------------------------------
def _args(**over):
    p = 0x10000  # never dereferenced: every call below is refused on its arguments
    a = dict(dist=p, goal=p, passable=p, grad_dist=p, B=2, H=70, W=130, neighbor_mask=0x1EF, grad_cost_out=p, status_out=p, visits_out=None,
             workspace=p, workspace_bytes=1 << 20, max_rounds=0, rounds_out=None, stream=None)
    a.update(over)
    return a


REFUSALS = [(dict(dist=None), 5), (dict(goal=None), 5), (dict(passable=None), 5), (dict(status_out=None), 5), (dict(workspace=None), 5),
            (dict(B=0), 1), (dict(H=0), 1), (dict(W=-1), 1),
            (dict(neighbor_mask=0x1FF), 2), (dict(neighbor_mask=0x200), 2),
            (dict(neighbor_mask=0x010, dist=None), 2),                        # the mask is looked at first
            (dict(dist=None, B=0), 5),                                         # a NULL before the shape
            (dict(B=0, H=1024, W=1153), 1),                                    # the shape before the limit
            (dict(H=1024, W=1153), 2), (dict(H=65536, W=65536), 2),
            (dict(B=1 << 23, H=70, W=130, workspace_bytes=1 << 50), 2),        # more than 2^24 tiles
            (dict(H=1024, W=1153, workspace_bytes=0), 2),                      # the limit before the workspace
            (dict(workspace_bytes=0), 6), (dict(workspace_bytes=15), 6),
            (dict(workspace=0x10004), 6), (dict(workspace=0x10001), 6)]        # off an 8-byte boundary: 4-byte aligned is not enough


@pytest.mark.parametrize("over,rc", REFUSALS + [(dict(grad_dist=None), 5), (dict(grad_cost_out=None), 5), (dict(max_rounds=-1), 1),
                                                (dict(max_rounds=-1, dist=None), 5), (dict(max_rounds=-1, H=1024, W=1153), 1)])
def test_fields_backward_tiled_refuses_bad_arguments_without_a_device(over, rc):
    from neural_astar import _native
    lib = _native.load()
    a = _args(**over)
    assert lib.nastar_fields_backward_tiled(*a.values()) == rc
    assert lib.nastar_fields_backward_tiled(*_args(visits_out=0x10000, **over).values()) == rc
    assert lib.nastar_last_error() == b""


@pytest.mark.parametrize("over,rc", REFUSALS)
def test_fields_backward_tiled_status_refuses_bad_arguments_without_a_device(over, rc):
    from neural_astar import _native
    lib = _native.load()
    a = _args(**over)
    keys = ("dist", "goal", "passable", "B", "H", "W", "neighbor_mask", "status_out", "workspace", "workspace_bytes", "stream")
    assert lib.nastar_fields_backward_tiled_status(*(a[k] for k in keys)) == rc
    assert lib.nastar_last_error() == b""


def test_short_workspace_is_measured_against_the_exported_size():
    from neural_astar import _native
    lib = _native.load()
    need = lib.nastar_fields_backward_tiled_workspace_bytes(2, 70, 130)
    assert need > 2 * 70 * 130 * 9
    assert lib.nastar_fields_backward_tiled(*_args(workspace_bytes=need - 1).values()) == 6
    a = _args(workspace_bytes=need - 1)
    assert lib.nastar_fields_backward_tiled_status(a["dist"], a["goal"], a["passable"], 2, 70, 130, 0x1EF, a["status_out"], a["workspace"], need - 1, None) == 6
    assert lib.nastar_last_error() == b""


# ---- 4: Python refusals without a device; the keyword -----------------------------------------------------------------------------------------------------
def test_ops_refuse_before_a_launch():
    from neural_astar import ops
    from neural_astar.planner import NeuralAstar, VanillaAstar
    from neural_astar.planner.differentiable_astar import DifferentiableAstar
    m = torch.ones(2, 1, 8, 8)
    big = torch.ones(1, 1, 128, 129)
    for t in (m, big):
        with pytest.raises(RuntimeError, match="HIP device"):
            ops.fields_backward_tiled(t, t, t, t)
        with pytest.raises(RuntimeError, match="HIP device"):
            ops.cost_to_go_tiled(t.clone().requires_grad_(True), t, t, differentiable=True)
        with pytest.raises(RuntimeError, match="HIP device"):
            ops.cost_to_go_tiled(t, t, t, differentiable=True)
        with pytest.raises(RuntimeError, match="HIP device"):
            DifferentiableAstar().cost_to_go_tiled(t, t, t, differentiable=True)
        with pytest.raises(RuntimeError, match="HIP device"):
            VanillaAstar().cost_to_go_tiled(t, t, differentiable=True)
    with pytest.raises(RuntimeError, match="HIP device"):
        NeuralAstar(encoder_arch="CNN").astar.cost_to_go_tiled(big, big, big)
    with pytest.raises(ValueError, match="share one"):
        ops.fields_backward_tiled(m, torch.ones(2, 1, 8, 9), m, m)
    with pytest.raises(ValueError, match="must be a"):
        ops.fields_backward_tiled(torch.ones(8, 8), m, m, m)
    with pytest.raises(TypeError, match="float32"):
        ops.fields_backward_tiled(m.double(), m.double(), m.double(), m)
    with pytest.raises(ValueError, match="neighbor_mask"):
        ops.fields_backward_tiled(m, m, m, m, neighbor_mask=0x1FF)
    for bad in (torch.ones(2, 1, 8, 9), torch.ones(2, 1, 8, 8, dtype=torch.float64), torch.ones(1, 1, 8, 8), None, torch.ones(2, 64)):
        with pytest.raises(ValueError, match="grad_dists"):
            ops.fields_backward_tiled(m, m, m, bad)
    for bad in (0, -3, 1.5, True):
        with pytest.raises(ValueError, match="max_rounds"):
            ops.fields_backward_tiled(m, m, m, m, max_rounds=bad)
        with pytest.raises(ValueError, match="max_rounds"):
            ops.cost_to_go_tiled(m, m, m, max_rounds=bad, differentiable=True)
    huge = torch.ones(1, 1, 1, 1).expand(1, 1, 1024, 1153)
    with pytest.raises(NotImplementedError, match="1179648"):
        ops.fields_backward_tiled(huge, huge, huge, huge)
    with pytest.raises(NotImplementedError, match="1179648"):
        ops.cost_to_go_tiled(huge, huge, huge, differentiable=True)
    with pytest.raises(ValueError, match="share one"):
        ops.cost_to_go_tiled(m, torch.ones(2, 1, 8, 9), m, differentiable=True)
    # the three pinned refusals keep their words and gain a hint
    with pytest.raises(NotImplementedError, match=r"tiled.*cost_to_go_tiled\(\.\.\., differentiable=True\)"):
        ops.cost_to_go(m, m, m, tiled=True, differentiable=True)
    with pytest.raises(NotImplementedError, match=r"16384.*cost_to_go_tiled\(\.\.\., differentiable=True\)"):
        ops.cost_to_go(big, big, big, differentiable=True)
    with pytest.raises(NotImplementedError, match=r"16384.*fields_backward_tiled"):
        ops.fields_backward(big, big, big, big)


def test_differentiable_is_the_last_keyword_and_defaults_to_false():
    from neural_astar import ops
    from neural_astar.planner import NeuralAstar, VanillaAstar
    from neural_astar.planner.differentiable_astar import DifferentiableAstar
    for fn in (ops.cost_to_go_tiled, DifferentiableAstar.cost_to_go_tiled, VanillaAstar.cost_to_go_tiled, NeuralAstar.cost_to_go_tiled):
        prm = list(inspect.signature(fn).parameters.values())
        assert prm[-1].name == "differentiable" and prm[-1].default is False, fn
        assert prm[-2].name in ("policies", "launches_per_batch")
    # the same leading arguments as the planners' cost_to_go
    for cls in (DifferentiableAstar, VanillaAstar, NeuralAstar):
        lead = [n for n in inspect.signature(cls.cost_to_go).parameters if n not in ("policies", "tiled", "differentiable")]
        assert [n for n in inspect.signature(cls.cost_to_go_tiled).parameters if n not in ("policies", "differentiable")] == lead, cls
    names = list(inspect.signature(ops.fields_backward_tiled).parameters)
    assert names == ["dists", "goal_maps", "obstacles_maps", "grad_dists", "neighbor_mask", "max_rounds", "visits_out"]
