"""CPU: the gradient of the cost-to-go field with respect to the cost maps (include/nastar_fields_grad.h, ``ops.cost_to_go(...,
differentiable=True)``) -- everything that needs no GPU.

1. the eighth header against ``_native.FIELD_GRAD_SIGNATURES``; the tables of the other headers are what they were;
2. the library exports the three symbols; abi and limit;
3. every refusal ``nastar_fields_backward`` makes before any HIP call, and their order;
4. the numpy definition (tests/fields_grad_oracle.py) against itself: a one-hot upstream gradient at n gives the roll-out from n
   (``MazeDataset.get_opt_traj``); subtree sizes on a corridor; what is not live is never read;
5. plateau detection on a zero-cost strip;
6. the Python refusals made before a launch, and the new keyword on the planner methods.
"""
import inspect
import os

import numpy as np
import pytest
import torch

import fields_grad_oracle as GO
import fields_oracle as FO
import heuristic_oracle as HO
from test_fields import _defines, _prototypes, random_map

f32 = np.float32


# ---- 1, 2: header, binding, library ---------------------------------------------------------------------------------------------------------------
def test_eighth_header_and_field_grad_signatures_agree():
    from neural_astar import _native
    protos = _prototypes("nastar_fields_grad.h")
    assert sorted(protos) == sorted(_native.FIELD_GRAD_SIGNATURES) == ["nastar_fields_backward", "nastar_fields_grad_abi", "nastar_fields_grad_max_cells"]
    for name, (ret, args) in protos.items():
        assert _native.FIELD_GRAD_SIGNATURES[name] == ret + " " + "".join(k for k, _ in args), name
    assert [n for _, n in protos["nastar_fields_backward"][1]] == ["dist", "goal", "passable", "grad_dist", "B", "H", "W", "neighbor_mask",
                                                                   "grad_cost_out", "status_out", "sweeps_out", "stream"]
    # a table of its own: the three tables tests/test_capi_library.py counts do not hold the new symbols
    for table in (_native.SIGNATURES, _native.FIELD_SIGNATURES, _native.TILED_FIELD_SIGNATURES):
        assert not set(_native.FIELD_GRAD_SIGNATURES) & set(table)
    assert len(_native.SIGNATURES) == 74 and len(_native.FIELD_SIGNATURES) == 4 and len(_native.TILED_FIELD_SIGNATURES) == 6
    new = _defines("nastar_fields_grad.h")
    assert new["NASTAR_FIELDS_GRAD_ABI"] == 1 and "NASTAR_VERSION" not in new and _defines("nastar.h")["NASTAR_VERSION"] == 800
    codes = {k: v for k, v in new.items() if k.startswith("NASTAR_ERR_")}
    assert codes == {"NASTAR_ERR_PLATEAU": 11} == {"NASTAR_ERR_PLATEAU": _native.NASTAR_ERR_PLATEAU} and GO.STATUS_PLATEAU == 11
    taken = {v for h in ("nastar.h", "nastar_fields.h") for k, v in _defines(h).items() if k == "NASTAR_OK" or k.startswith("NASTAR_ERR_")}
    assert 11 not in taken and max(taken) == 10


def test_library_exports_the_field_grad_symbols():
    from neural_astar import _native, ops
    lib = _native.load()
    for sym in _native.FIELD_GRAD_SIGNATURES:
        assert hasattr(lib, sym), sym
    assert lib.nastar_fields_grad_abi() == 1
    assert lib.nastar_fields_grad_max_cells() == ops.FIELDS_GRAD_MAX_CELLS == ops.FIELDS_MAX_CELLS == 16384
    assert len(lib.nastar_fields_backward.argtypes) == 12
    assert ops.FIELD_PLATEAU == _native.NASTAR_ERR_PLATEAU == 11
    assert {"fields_backward", "FIELD_PLATEAU", "FIELDS_GRAD_MAX_CELLS", "cost_to_go"} <= set(ops.__all__)


# ---- 3: refusals, made before any HIP call -----------------------------------------------------------------------------------------------------------
def _args(**over):
    p = 0x10000  # never dereferenced: every call below is refused on its arguments
    a = dict(dist=p, goal=p, passable=p, grad_dist=p, B=2, H=8, W=8, neighbor_mask=0x1EF, grad_cost_out=p, status_out=p, sweeps_out=None, stream=None)
    a.update(over)
    return a


@pytest.mark.parametrize("over,rc", [(dict(dist=None), 5), (dict(goal=None), 5), (dict(passable=None), 5), (dict(grad_dist=None), 5),
                                     (dict(grad_cost_out=None), 5), (dict(status_out=None), 5), (dict(B=0), 1), (dict(H=0), 1), (dict(W=-1), 1),
                                     (dict(neighbor_mask=0x1FF), 2), (dict(neighbor_mask=0x200), 2),
                                     (dict(neighbor_mask=0x010, dist=None), 2),       # the mask is looked at first
                                     (dict(dist=None, B=0), 5),                        # a NULL before the shape
                                     (dict(B=0, H=128, W=129), 1),                     # the shape before the limit
                                     (dict(H=128, W=129), 2), (dict(H=1, W=16385), 2), (dict(H=65536, W=65536), 2)])
def test_fields_backward_refuses_bad_arguments_without_a_device(over, rc):
    from neural_astar import _native
    lib = _native.load()
    assert lib.nastar_fields_backward(*_args(**over).values()) == rc
    assert lib.nastar_fields_backward(*_args(sweeps_out=0x10000, **over).values()) == rc
    assert lib.nastar_last_error() == b""


# ---- 4: the definition against itself -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,mask", [(16, 16, HO.MOORE8), (20, 45, HO.MOORE8), (18, 22, HO.VON_NEUMANN), (24, 24, 0x0EB)])
def test_one_hot_gradient_is_the_roll_out(H, W, mask):
    from neural_astar.utils.data import MazeDataset
    rng = np.random.default_rng(H * 7 + W)
    cost, passable, goal = random_map(rng, H, W, 0.25)
    cost = (cost + 0.5).astype(f32)
    d, pol, _ = FO.field(cost, goal, passable, mask)
    live = np.argwhere(np.isfinite(d) & (goal == 0))
    assert len(live) > 4
    for y, x in live[rng.permutation(len(live))[:8]]:
        G = np.zeros((H, W), f32)
        G[y, x] = 1
        r = GO.field_grad(cost, goal, passable, G, mask)
        start = np.zeros((1, H, W), f32)
        start[0, y, x] = 1
        traj = MazeDataset.get_opt_traj(None, start, goal[None], pol)[0]
        assert r.status == 0 and np.array_equal(r.grad, traj) and r.grad.sum() == r.hops[y, x] >= 1


def test_subtree_sizes_on_a_corridor_and_dead_cells_are_never_read():
    # one row, the goal at the right end, a wall in the middle: cells left of the wall reach nothing
    W = 9
    cost = np.full((1, W), 0.75, f32)
    passable = np.ones((1, W), f32)
    passable[0, 3] = 0
    goal = np.zeros((1, W), f32)
    goal[0, 8] = 1
    G = np.ones((1, W), f32)
    G[0, [0, 1, 2, 3, 8]] = [np.nan, np.inf, -np.inf, np.nan, np.nan]   # unreachable, obstacle, goal
    r = GO.field_grad(cost, goal, passable, G)
    assert r.status == 0 and r.live[0].tolist() == [False] * 4 + [True] * 4 + [False]
    assert r.grad[0].tolist() == [0, 0, 0, 0, 1, 2, 3, 4, 0] and r.hops[0].tolist() == [0, 0, 0, 0, 4, 3, 2, 1, 0]
    assert r.succ[0].tolist() == [-1, -1, -1, -1, 5, 6, 7, 8, -1]
    # sum(grad * cost) is the sum of the field over the live cells (G = 1): every cell pays its cost once per roll-out through it
    assert float((r.grad * cost).sum()) == float(r.dist[r.live].sum()) == 0.75 * 10
    none = GO.field_grad(cost, np.zeros((1, W), f32), passable, G)   # no goal: nothing is live
    assert none.status == 0 and not none.live.any() and not none.grad.any()


# ---- 5: plateaus ----------------------------------------------------------------------------------------------------------------------------------------
def test_zero_cost_strip_is_a_plateau():
    H, W = 5, 7
    cost = np.ones((H, W), f32)
    passable, goal = np.ones((H, W), f32), np.zeros((H, W), f32)
    goal[2, 6] = 1
    G = np.ones((H, W), f32)
    assert GO.field_grad(cost, goal, passable, G).status == 0
    cost[2, 2:5] = 0                       # cells that cost nothing: D(n) = 0 + D(m), the best neighbour is not strictly closer
    r = GO.field_grad(cost, goal, passable, G)
    assert r.status == GO.STATUS_PLATEAU == 11 and not r.grad.any() and r.grad.dtype == f32
    assert ((r.succ < 0) & r.live).sum() == 3
    # a zero-cost cell beside the goal has D == 0 and is not a goal: live, with nothing below it
    beside = np.ones((H, W), f32)
    beside[2, 5] = 0
    r = GO.field_grad(beside, goal, passable, G)
    assert r.status == 11 and r.dist[2, 5] == 0 and r.live[2, 5]
    # a cost the addition absorbs: fl32(2^-30 + 2) == 2 does not rise above the neighbour's 2
    tiny = np.ones((H, W), f32)
    tiny[2, 3] = 2.0 ** -30
    r = GO.field_grad(tiny, goal, passable, G)
    assert r.status == 11 and r.dist[2, 3] == r.dist[2, 4] == 2 and r.succ[2, 3] < 0


# ---- 6: Python refusals before a launch; the keyword on every planner method ------------------------------------------------------------------------
def test_differentiable_keyword_and_refusals_before_a_launch():
    from neural_astar import ops
    from neural_astar.planner import NeuralAstar, VanillaAstar
    from neural_astar.planner.differentiable_astar import DifferentiableAstar
    for fn in (ops.cost_to_go, DifferentiableAstar.cost_to_go, VanillaAstar.cost_to_go, NeuralAstar.cost_to_go):
        prm = list(inspect.signature(fn).parameters.values())[-1]
        assert prm.name == "differentiable" and prm.default is False, fn
    m = torch.ones(2, 1, 8, 8, requires_grad=True)
    with pytest.raises(NotImplementedError, match="tiled"):
        ops.cost_to_go(m, m, m, tiled=True, differentiable=True)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.cost_to_go(m, m, m, differentiable=True)
    with pytest.raises(ValueError, match="share one"):
        ops.cost_to_go(m, torch.ones(2, 1, 8, 9), m, differentiable=True)
    with pytest.raises(ValueError, match="neighbor_mask"):
        ops.cost_to_go(m, m, m, neighbor_mask=0x1FF, differentiable=True)
    big = torch.ones(1, 1, 128, 129)
    with pytest.raises(NotImplementedError, match="16384"):
        ops.cost_to_go(big, big, big, differentiable=True)
    with pytest.raises(NotImplementedError, match="16384"):
        ops.fields_backward(big, big, big, big)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.fields_backward(m.detach(), m.detach(), m.detach(), m.detach())
    with pytest.raises(ValueError, match="grad_dists"):
        ops.fields_backward(m.detach(), m.detach(), m.detach(), torch.ones(2, 1, 8, 9))
    with pytest.raises(RuntimeError, match="HIP device"):
        VanillaAstar().cost_to_go(m, m, differentiable=True)
    with pytest.raises(NotImplementedError, match="tiled"):
        DifferentiableAstar().cost_to_go(m, m, m, tiled=True, differentiable=True)
