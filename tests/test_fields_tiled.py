"""CPU: the tiled cost-to-go relaxation (include/nastar_fields_tiled.h, ``ops.cost_to_go_tiled``) -- everything that needs no GPU.

1. the numpy restatement of the tiled scheme (tests/fields_tiled_oracle.py: random tile order, every halo cell fresh or one round stale at
   random) equals the definition (tests/fields_oracle.py) bit for bit;
2. the init trap: a goal in a tile's corner cell, walled in inside its own tile, still reaches the neighbouring tiles -- and does not under
   the rule "mark the tile that holds the goal";
3. a round budget that is too small: status 10, upper bounds, finite only where the field is;
4. the sixth header against ``_native.TILED_FIELD_SIGNATURES``, disjoint from the other tables;
5. refusals made before any launch; the default ``cost_to_go`` above its limit raises as before.
"""
import numpy as np
import pytest
import torch

import fields_oracle as FO
import fields_tiled_oracle as TO
import heuristic_oracle as HO
from test_fields import _defines, _prototypes

f32 = np.float32


def _random(rng, H, W, kind, p_obstacle=0.3):
    passable = (rng.random((H, W)) > p_obstacle).astype(f32)
    goal = np.zeros((H, W), f32)
    gy, gx = int(rng.integers(H)), int(rng.integers(W))
    goal[gy, gx] = passable[gy, gx] = 1
    cost = passable.copy() if kind == "binary" else np.zeros((H, W), f32) if kind == "zero" else rng.random((H, W)).astype(f32)
    return cost, goal, passable


# ---- 1: fresh or stale halos, any tile order: the same bits ---------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,tile,kind,mask", [
    (33, 47, (16, 16), "u1", HO.MOORE8), (33, 47, (16, 16), "binary", HO.VON_NEUMANN), (33, 47, (16, 16), "zero", HO.MOORE8),
    (33, 47, (16, 16), "u1", 0x0EB), (65, 65, (64, 64), "u1", HO.MOORE8), (65, 65, (64, 64), "binary", HO.VON_NEUMANN),
    (70, 130, (64, 64), "u1", HO.VON_NEUMANN), (70, 130, (64, 64), "zero", HO.MOORE8), (129, 128, (64, 64), "u1", HO.MOORE8),
    (130, 259, (64, 64), "binary", HO.MOORE8), (200, 200, (64, 64), "u1", HO.MOORE8)])
def test_tiled_scheme_is_the_definition(H, W, tile, kind, mask):
    rng = np.random.default_rng([H, W, mask])
    cost, goal, passable = _random(rng, H, W, kind)
    want, _, status = FO.field(cost, goal, passable, mask)
    got, st, rounds, visits = TO.tiled_field(cost, goal, passable, mask, tile, rng)
    assert st == status == 0 and np.array_equal(got, want)
    plain, st2, rounds2, _ = TO.tiled_field(cost, goal, passable, mask, tile)      # every halo fresh, tiles in index order
    assert st2 == 0 and np.array_equal(plain, want)
    print(f"{H}x{W} {kind} {hex(mask)}: {rounds} rounds, {visits} tile visits with random halos; {rounds2} rounds with fresh ones")
    assert 1 <= rounds <= H * W + 1 and visits >= rounds


@pytest.mark.parametrize("H,W,tile", [(33, 47, (16, 16)), (65, 65, (64, 64)), (70, 130, (64, 64))])
def test_tiled_scheme_on_a_serpentine(H, W, tile):
    cost, goal, passable, walls = TO.serpentine(H, W)
    want, _, _ = FO.field(cost, goal, passable)
    got, st, rounds, _ = TO.tiled_field(cost, goal, passable, HO.MOORE8, tile, np.random.default_rng(H))
    assert st == 0 and np.array_equal(got, want) and np.isfinite(want[passable != 0]).all()
    assert want.max() > walls * (W - 2)                 # every corridor is run from end to end
    assert rounds >= walls // 2


def test_no_goal_and_bad_cost():
    rng = np.random.default_rng(3)
    cost, goal, passable = _random(rng, 33, 47, "u1")
    got, st, rounds, visits = TO.tiled_field(cost, np.zeros_like(goal), passable, tile=(16, 16))
    assert st == FO.STATUS_NO_GOAL and np.isinf(got).all() and rounds == visits == 0
    cost[np.nonzero(passable)[0][0], np.nonzero(passable)[1][0]] = -1
    got, st, _, _ = TO.tiled_field(cost, goal, passable, tile=(16, 16))
    assert st == FO.STATUS_BAD_COST and np.isinf(got).all()


# ---- 2: the init trap ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("corner", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_walled_in_corner_goal_reaches_the_neighbouring_tiles(corner):
    th = tw = 16
    H, W = 3 * th, 3 * tw
    cost, passable, goal = np.ones((H, W), f32), np.ones((H, W), f32), np.zeros((H, W), f32)
    gy, gx = th + corner[0] * (th - 1), tw + corner[1] * (tw - 1)     # a corner cell of the interior tile (1, 1)
    goal[gy, gx] = 1
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            y, x = gy + dy, gx + dx
            if (dy or dx) and th <= y < 2 * th and tw <= x < 2 * tw:
                passable[y, x] = 0                                    # its neighbours inside its own tile
    want, _, _ = FO.field(cost, goal, passable)
    assert np.isfinite(want[passable != 0]).all()
    got, st, _, _ = TO.tiled_field(cost, goal, passable, tile=(th, tw), rng=np.random.default_rng(5))
    assert st == 0 and np.array_equal(got, want)
    wrong, _, rounds, _ = TO.tiled_field(cost, goal, passable, tile=(th, tw), init="own")
    assert rounds == 1 and np.isinf(np.delete(wrong.reshape(-1), gy * W + gx)).all()   # the trap: the goal's own tile lowers nothing


# ---- 3: a round budget that is too small -----------------------------------------------------------------------------------------------------
def test_too_few_rounds_leave_upper_bounds():
    cost, goal, passable, _ = TO.serpentine(65, 65)
    want, _, _ = FO.field(cost, goal, passable)
    got, st, rounds, _ = TO.tiled_field(cost, goal, passable, tile=(64, 64), rng=np.random.default_rng(1), max_rounds=2)
    assert st == TO.STATUS_NO_CONVERGENCE and rounds == 2
    assert (got >= want).all() and not (np.isfinite(got) & ~np.isfinite(want)).any() and (got > want).any()


# ---- 4: header and binding --------------------------------------------------------------------------------------------------------------------
def test_sixth_header_and_tiled_field_signatures_agree():
    from neural_astar import _native
    protos = _prototypes("nastar_fields_tiled.h")
    assert sorted(protos) == sorted(_native.TILED_FIELD_SIGNATURES)
    assert {"nastar_fields_tiled_abi", "nastar_fields_tiled_max_cells", "nastar_fields_tile", "nastar_cost_to_go_tiled_workspace_bytes",
            "nastar_cost_to_go_tiled"} <= set(protos)
    for name, (ret, args) in protos.items():
        assert _native.TILED_FIELD_SIGNATURES[name] == ret + " " + "".join(k for k, _ in args), name
    assert [n for _, n in protos["nastar_cost_to_go_tiled"][1]] == ["cost", "goal", "passable", "B", "H", "W", "neighbor_mask", "dist_out", "policy_out",
                                                                    "status_out", "visits_out", "workspace", "workspace_bytes", "max_rounds",
                                                                    "rounds_out", "stream"]
    for other in (_native.SIGNATURES, _native.ROUTE_SIGNATURES, _native.SOURCE_SIGNATURES, _native.LEVEL_SIGNATURES, _native.FIELD_SIGNATURES):
        assert not set(_native.TILED_FIELD_SIGNATURES) & set(other)
    # the other headers and their tables are what they were
    assert len(_prototypes("nastar.h")) == len(_native.SIGNATURES) == 74 and len(_prototypes("nastar_fields.h")) == len(_native.FIELD_SIGNATURES) == 4
    new = _defines("nastar_fields_tiled.h")
    assert new == {"NASTAR_FIELDS_TILED_ABI": 1} and _defines("nastar_fields.h")["NASTAR_FIELDS_ABI"] == 1


def test_library_exports_the_tiled_symbols():
    from neural_astar import _native, ops
    lib = _native.load()
    for sym in _native.TILED_FIELD_SIGNATURES:
        assert hasattr(lib, sym), sym
    assert lib.nastar_fields_tiled_abi() == 1
    assert lib.nastar_fields_tiled_max_cells() == ops.FIELDS_TILED_MAX_CELLS == 1024 * 1152
    th, tw = ops.fields_tile()
    assert th >= 1 and tw >= 1
    assert lib.nastar_fields_tile(None, None) == 5
    ws = lib.nastar_cost_to_go_tiled_workspace_bytes
    tiles = -(-130 // th) * -(-259 // tw)
    assert ws(3, 130, 259) >= 3 * 16 + 2 * 4 * 3 * tiles and ws(3, 130, 259) % 16 == 0
    assert ws(1, 1024, 1152) > 0 and ws(1, 1024, 1153) == 0 and ws(0, 8, 8) == 0 and ws(1, 0, 8) == 0
    assert ws(1 << 24, th, tw) > 0 and ws((1 << 24) + 1, th, tw) == 0 and ws(1 << 23, th + 1, tw + 1) == 0   # at most 2^24 tiles in a batch
    assert len(lib.nastar_cost_to_go_tiled.argtypes) == 16


# ---- 5: refusals, made before any launch ---------------------------------------------------------------------------------------------------------
def _tiled_args(**over):
    p = 0x10000  # never dereferenced: every call below is refused on its arguments
    a = dict(cost=p, goal=p, passable=p, B=2, H=70, W=130, neighbor_mask=0x1EF, dist_out=p, policy_out=None, status_out=p, visits_out=None,
             workspace=p, workspace_bytes=1 << 20, max_rounds=0, rounds_out=None, stream=None)
    a.update(over)
    return a


@pytest.mark.parametrize("over,rc", [(dict(cost=None), 5), (dict(goal=None), 5), (dict(passable=None), 5), (dict(dist_out=None), 5),
                                     (dict(status_out=None), 5), (dict(workspace=None), 5), (dict(B=0), 1), (dict(H=0), 1), (dict(W=-1), 1),
                                     (dict(max_rounds=-1), 1), (dict(neighbor_mask=0x1FF), 2), (dict(neighbor_mask=0x200), 2),
                                     (dict(neighbor_mask=0x010, cost=None), 2), (dict(H=1024, W=1153), 2), (dict(H=1, W=1024 * 1152 + 1), 2),
                                     (dict(H=65536, W=65536), 2), (dict(workspace_bytes=0), 6), (dict(workspace_bytes=15), 6), (dict(workspace=0x10002), 6),
                                     (dict(B=1 << 23, H=70, W=130, workspace_bytes=1 << 40), 2)])
def test_cost_to_go_tiled_refuses_bad_arguments_without_a_device(over, rc):
    from neural_astar import _native
    lib = _native.load()
    a = _tiled_args(**over)
    assert lib.nastar_cost_to_go_tiled(*a.values()) == rc
    v = list(a.values())
    assert lib.nastar_cost_to_go_tiled_batched(*v[:14], 0, *v[14:]) == rc
    assert rc != 6 or a["workspace"] % 4 or lib.nastar_cost_to_go_tiled_workspace_bytes(a["B"], a["H"], a["W"]) > a["workspace_bytes"]


def test_short_workspace_is_measured_against_the_exported_size():
    from neural_astar import _native
    lib = _native.load()
    need = lib.nastar_cost_to_go_tiled_workspace_bytes(2, 70, 130)
    assert lib.nastar_cost_to_go_tiled(*_tiled_args(workspace_bytes=need - 1).values()) == 6
    assert lib.nastar_cost_to_go_tiled_batched(*list(_tiled_args().values())[:14], -1, None, None) == 1


def test_ops_refuse_before_a_launch():
    from neural_astar import ops
    from neural_astar.planner import NeuralAstar, VanillaAstar
    from neural_astar.planner.differentiable_astar import DifferentiableAstar
    m = torch.ones(2, 1, 8, 8)
    big = torch.ones(1, 1, 128, 129)
    for t in (m, big):
        with pytest.raises(RuntimeError, match="HIP device"):
            ops.cost_to_go(t, t, t, tiled=True)
        with pytest.raises(RuntimeError, match="HIP device"):
            ops.cost_to_go_tiled(t, t, t)
        with pytest.raises(RuntimeError, match="HIP device"):
            DifferentiableAstar().cost_to_go(t, t, t, tiled=True)
        with pytest.raises(RuntimeError, match="HIP device"):
            VanillaAstar().cost_to_go(t, t, tiled=True)
    with pytest.raises(RuntimeError, match="HIP device"):
        NeuralAstar(encoder_arch="CNN").astar.cost_to_go(big, big, big, tiled=True)
    with pytest.raises(ValueError, match="share one"):
        ops.cost_to_go_tiled(m, torch.ones(2, 1, 8, 9), m)
    with pytest.raises(ValueError, match="neighbor_mask"):
        ops.cost_to_go_tiled(m, m, m, neighbor_mask=0x1FF)
    with pytest.raises(TypeError, match="float32"):
        ops.cost_to_go_tiled(m.double(), m.double(), m.double())
    for bad in (0, -3, 1.5, True):
        with pytest.raises(ValueError, match="max_rounds"):
            ops.cost_to_go_tiled(m, m, m, max_rounds=bad)
    with pytest.raises(ValueError, match="sweeps_out"):
        ops.cost_to_go(m, m, m, tiled=True, sweeps_out=torch.zeros(2, dtype=torch.int32))
    huge = torch.ones(1, 1, 1, 1).expand(1, 1, 1024, 1153)
    with pytest.raises(NotImplementedError, match="1179648"):
        ops.cost_to_go_tiled(huge, huge, huge)


def test_default_cost_to_go_above_its_limit_raises_as_before():
    from neural_astar import ops
    from neural_astar.planner import VanillaAstar
    big = torch.ones(1, 1, 128, 129)
    with pytest.raises(NotImplementedError, match="16384"):
        ops.cost_to_go(big, big, big)
    with pytest.raises(NotImplementedError, match="16384"):
        ops.cost_to_go(big, big, big, tiled=False)
    with pytest.raises(NotImplementedError, match="16384"):
        VanillaAstar().cost_to_go(big, big)
    assert ops.FIELDS_MAX_CELLS == 16384
