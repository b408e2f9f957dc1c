"""CPU: cost-to-go fields and optimal policies (include/nastar_fields.h, ``ops.cost_to_go``) -- everything that needs no GPU.

1-2. the numpy definition (tests/fields_oracle.py) against ``synthetic.geodesic_distance`` / ``optimal_policies`` and the maze fixture;
3.   order independence: Jacobi against a randomly ordered in-place relaxation, bit for bit;
4.   against float64 Dijkstra (scipy) on the reversed graph;
5.   the identity that ties the field to the search: a Dijkstra-mode search's route cost is the field at its start, exactly;
6.   the fifth header against ``_native.FIELD_SIGNATURES``; nastar.h keeps its 74 symbols; the new status codes collide with none of its;
7.   refusals made before any launch.
"""
import os
import re

import numpy as np
import pytest
import torch

import fields_oracle as FO
import heuristic_oracle as HO
import route_oracle as RO
from neural_astar.utils import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
MASKS = [HO.MOORE8, HO.VON_NEUMANN, 0x0EB, 0x1A7, 0x04F, 0x1E6]


def random_map(rng, H, W, p_obstacle=0.3, scale=1.0, dyadic=False):
    """cost, passable (bool), goal (one-hot f32 on a passable cell)"""
    passable = rng.random((H, W)) > p_obstacle
    passable[tuple(rng.integers(0, (H, W)))] = True
    free = np.argwhere(passable)
    goal = np.zeros((H, W), f32)
    goal[tuple(free[rng.integers(len(free))])] = 1
    cost = (rng.integers(1, 257, (H, W)) / 64.0).astype(f32) if dyadic else (rng.random((H, W)) * scale).astype(f32)
    return cost, passable, goal


# ---- 1, 2: the definition reproduces the host path and the fixture ---------------------------------------------------------------------------
@pytest.mark.parametrize("problems", ["maze", "random"])
def test_oracle_is_the_host_path_on_unit_cost(problems):
    P = syn.maze_maps(6, 32, seed=5) if problems == "maze" else syn.random_obstacle_maps(6, 20, 45, 0.3, seed=9)
    ok = P.map_designs[:, 0] > 0
    B = ok.shape[0]
    gi = P.goal_maps.reshape(B, -1).argmax(1)
    bfs = syn.geodesic_distance(ok, gi)
    d, pol, st = FO.fields(P.map_designs, P.goal_maps, P.map_designs)
    assert (st == 0).all()
    assert np.array_equal(d, np.where(bfs >= 0, bfs.astype(f32), f32(np.inf)))
    assert np.array_equal(pol, syn.optimal_policies(ok, bfs)[:, :, 0])
    if problems == "random":
        assert np.isinf(d[ok]).any(), "the random maps were meant to hold walled-in passable cells"


@pytest.mark.parametrize("split", [0, 4, 8])
def test_oracle_reproduces_the_maze_fixture(split):
    with np.load(os.path.join(ROOT, "tests", "golden", "data_maze32.npz")) as z:
        maps, goals, pols, dists = (z[f"arr_{split + k}"] for k in range(4))
    d, pol, st = FO.fields(maps, goals, maps)
    assert (st == 0).all()
    worst = np.where(np.isfinite(d), d, 0).max((1, 2), keepdims=True)
    assert np.array_equal(np.where(np.isfinite(d), -d, -(worst + 1)).astype(f32), dists[:, 0])
    assert np.array_equal(pol, pols[:, :, 0])


# ---- 3: the order of the updates does not matter ----------------------------------------------------------------------------------------------
def chaotic(cost, passable, goal, mask, rng):
    H, W = cost.shape
    moves = HO.offsets(mask)
    r = np.where((goal != 0) & passable, f32(0), f32(np.inf)).astype(f32)
    cells = [(y, x) for y in range(H) for x in range(W) if passable[y, x]]
    changed = True
    while changed:
        changed = False
        rng.shuffle(cells)
        for y, x in cells:
            best = f32(np.inf)
            for dy, dx in moves:
                if 0 <= y + dy < H and 0 <= x + dx < W:
                    best = min(best, r[y + dy, x + dx])
            v = f32(cost[y, x] + best)
            if v < r[y, x]:
                r[y, x] = v
                changed = True
    return np.where(goal != 0, f32(0), r)


@pytest.mark.parametrize("H,W,mask", [(16, 16, HO.MOORE8), (7, 5, HO.VON_NEUMANN), (20, 45, 0x0EB), (18, 22, HO.MOORE8)])
def test_relaxation_order_does_not_change_a_bit(H, W, mask):
    rng = np.random.default_rng(H * 100 + W)
    cost, passable, goal = random_map(rng, H, W)
    d, _, _ = FO.field(cost, goal, passable, mask)
    assert np.array_equal(d, chaotic(cost, passable, goal, mask, rng))


# ---- 4: float64 Dijkstra ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,scale,mask", [(16, 16, 1.0, HO.MOORE8), (12, 20, 1.0, HO.VON_NEUMANN), (7, 5, 10.0, HO.MOORE8), (24, 24, 1.0, 0x1A7),
                                            (32, 32, 0.05, HO.MOORE8), (20, 45, 1.0, HO.MOORE8)])
def test_oracle_against_float64_dijkstra(H, W, scale, mask):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import dijkstra
    rng = np.random.default_rng(H + W)
    cost, passable, goal = random_map(rng, H, W, scale=scale)
    rows, cols, w = [], [], []
    for y in range(H):
        for x in range(W):
            if passable[y, x]:
                for dy, dx in HO.offsets(mask):
                    if 0 <= y + dy < H and 0 <= x + dx < W and passable[y + dy, x + dx]:
                        # the move n -> m costs cost[n]; distances TO the goal are distances FROM it on the reversed graph (m -> n)
                        rows.append((y + dy) * W + x + dx)
                        cols.append(y * W + x)
                        w.append(float(cost[y, x]) + 1e-300)  # (a stored zero would not be an edge)
    ref = dijkstra(coo_matrix((w, (rows, cols)), shape=(H * W, H * W)).tocsr(), indices=int(goal.reshape(-1).argmax())).reshape(H, W)
    d, _, _ = FO.field(cost, goal, passable, mask)
    fin = np.isfinite(d)
    assert np.array_equal(fin, np.isfinite(ref))
    err = np.abs(d[fin] - ref[fin]).max()
    print(f"{H}x{W}: max |fp32 field - float64 Dijkstra| = {err:.3e}, largest distance {ref[fin].max():.3f}")
    assert err <= H * W * 2.0 ** -24 * ref[fin].max()


# ---- 5: the field is what a Dijkstra-mode search pays ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,mask", [(7, 5, HO.MOORE8), (16, 16, 0x0EB), (12, 20, 0x1A7), (9, 14, 0x04F), (24, 24, 0x1E6), (16, 16, HO.VON_NEUMANN),
                                      (20, 21, HO.MOORE8), (24, 24, HO.VON_NEUMANN)])
def test_dijkstra_mode_route_cost_is_the_field_at_the_start(H, W, mask):
    rng = np.random.default_rng(H * 31 + W + mask)
    solved = 0
    for trial in range(4):
        cost, passable, goal = random_map(rng, H, W, 0.25, dyadic=True)
        d, _, _ = FO.field(cost, goal, passable, mask)
        # any passable start on even trials (an asymmetric move set leaves most without a route), one with a route on odd trials
        free = np.argwhere(passable if trial % 2 == 0 or not (np.isfinite(d) & (d > 0)).any() else np.isfinite(d) & (d > 0))
        s = tuple(free[rng.integers(len(free))])
        start = np.zeros((1, H, W), f32)
        start[0][s] = 1
        r = RO.plan(cost[None], start, goal[None], passable[None].astype(f32), 1.0, H * W, mask, h0=np.zeros((1, H, W), f32))
        assert (r.status[0] != 0) == bool(np.isinf(d[s]))
        if r.status[0] == 0:
            assert f32(r.costs[0]) == d[s] and r.costs[0] == float(d[s])
            solved += 1
    assert solved


# ---- 6: header and binding ----------------------------------------------------------------------------------------------------------------------
_SCALARS = {"int": "i", "unsigned": "u", "float": "f", "double": "d", "size_t": "z", "long long": "q"}


def _prototypes(header):
    """include/<header> -> {symbol: (return letter, [(kind letter, parameter name), ...])} in the letters of _native.SIGNATURES"""
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    txt = re.sub(r"^\s*#.*$", "", txt, flags=re.M)
    out = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w \*]*?)\s*\b(nastar_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", txt):
        args = []
        for prm in (x.strip() for x in params.split(",")):
            if prm == "void":
                continue
            typ, arg = re.fullmatch(r"(.*?)(\w+)", prm).groups()
            base = " ".join(w for w in typ.replace("*", " ").split() if w != "const")
            args.append(("p" if "*" in typ else _SCALARS[base], arg))
        out[name] = ({"int": "i", "size_t": "z"}.get(ret.strip(), "s"), args)
    return out


def _defines(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    return {k: int(v, 0) for k, v in re.findall(r"^#define (NASTAR_\w+) (-?(?:0x)?[0-9A-Fa-f]+)\b", txt, flags=re.M)}


def test_fifth_header_and_field_signatures_agree():
    from neural_astar import _native
    protos = _prototypes("nastar_fields.h")
    assert sorted(protos) == sorted(_native.FIELD_SIGNATURES)
    assert {"nastar_fields_abi", "nastar_fields_max_cells", "nastar_cost_to_go"} <= set(protos)
    for name, (ret, args) in protos.items():
        assert _native.FIELD_SIGNATURES[name] == ret + " " + "".join(k for k, _ in args), name
    assert [n for _, n in protos["nastar_cost_to_go"][1]] == ["cost", "goal", "passable", "B", "H", "W", "neighbor_mask", "dist_out", "policy_out",
                                                              "status_out", "stream"]
    assert not set(_native.FIELD_SIGNATURES) & set(_native.SIGNATURES)
    # nastar.h and its table are what they were
    assert len(_prototypes("nastar.h")) == len(_native.SIGNATURES) == 74
    old, new = _defines("nastar.h"), _defines("nastar_fields.h")
    assert new["NASTAR_FIELDS_ABI"] == 1 and "NASTAR_VERSION" not in new and old["NASTAR_VERSION"] == 800
    old_codes = {v for k, v in old.items() if k == "NASTAR_OK" or k.startswith("NASTAR_ERR_")}
    new_codes = {k: v for k, v in new.items() if k.startswith("NASTAR_ERR_")}
    assert sorted(new_codes) == ["NASTAR_ERR_BAD_COST", "NASTAR_ERR_NO_CONVERGENCE"] and not set(new_codes) & set(old)
    assert len(set(new_codes.values())) == 2 and not set(new_codes.values()) & old_codes
    assert (_native.NASTAR_ERR_BAD_COST, _native.NASTAR_ERR_NO_CONVERGENCE) == (new["NASTAR_ERR_BAD_COST"], new["NASTAR_ERR_NO_CONVERGENCE"])
    assert FO.STATUS_BAD_COST == new["NASTAR_ERR_BAD_COST"] and FO.STATUS_NO_GOAL == old["NASTAR_ERR_UNSOLVABLE"] == 3


def test_library_exports_the_field_symbols():
    from neural_astar import _native, ops
    lib = _native.load()
    for sym in _native.FIELD_SIGNATURES:
        assert hasattr(lib, sym), sym
    assert lib.nastar_fields_abi() == 1
    assert lib.nastar_fields_max_cells() == ops.FIELDS_MAX_CELLS == 16384
    assert len(lib.nastar_cost_to_go.argtypes) == 11
    assert (ops.FIELD_BAD_COST, ops.FIELD_NO_CONVERGENCE) == (_native.NASTAR_ERR_BAD_COST, _native.NASTAR_ERR_NO_CONVERGENCE)


# ---- 7: refusals, made before any launch --------------------------------------------------------------------------------------------------------
def _field_args(**over):
    p = 0x10000  # never dereferenced: every call below is refused on its arguments
    a = dict(cost=p, goal=p, passable=p, B=2, H=8, W=8, neighbor_mask=0x1EF, dist_out=p, policy_out=None, status_out=p, stream=None)
    a.update(over)
    return a


@pytest.mark.parametrize("over,rc", [(dict(cost=None), 5), (dict(goal=None), 5), (dict(passable=None), 5), (dict(dist_out=None), 5),
                                     (dict(status_out=None), 5), (dict(B=0), 1), (dict(H=0), 1), (dict(W=-1), 1),
                                     (dict(neighbor_mask=0x1FF), 2), (dict(neighbor_mask=0x200), 2), (dict(neighbor_mask=0x010, cost=None), 2),
                                     (dict(H=128, W=129), 2), (dict(H=1, W=16385), 2), (dict(H=65536, W=65536), 2)])
def test_cost_to_go_refuses_bad_arguments_without_a_device(over, rc):
    from neural_astar import _native
    lib = _native.load()
    assert lib.nastar_cost_to_go(*_field_args(**over).values()) == rc
    a = _field_args(**over)
    assert lib.nastar_cost_to_go_sweeps(*list(a.values())[:-1], None, a["stream"]) == rc


def test_ops_cost_to_go_refuses_before_a_launch():
    from neural_astar import ops
    from neural_astar.planner import NeuralAstar, VanillaAstar
    from neural_astar.planner.astar import FieldOutput
    from neural_astar.planner.differentiable_astar import DifferentiableAstar, FieldOutput as F2
    assert FieldOutput is F2 is ops.FieldOutput and FieldOutput._fields == ("dists", "policies", "status")
    m = torch.ones(2, 1, 8, 8)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.cost_to_go(m, m, m)
    with pytest.raises(ValueError, match="share one"):
        ops.cost_to_go(m, torch.ones(2, 1, 8, 9), m)
    with pytest.raises(ValueError, match="share one"):
        ops.cost_to_go(m, m, torch.ones(3, 1, 8, 8))
    with pytest.raises(ValueError, match="must be a"):
        ops.cost_to_go(torch.ones(8, 8), m, m)
    for bad in (0x1FF, 0x200, -1, 0x10, 1.5, True):
        with pytest.raises(ValueError, match="neighbor_mask"):
            ops.cost_to_go(m, m, m, neighbor_mask=bad)
    big = torch.ones(1, 1, 128, 129)
    with pytest.raises(NotImplementedError, match="16384"):
        ops.cost_to_go(big, big, big)
    with pytest.raises(TypeError, match="float32"):
        ops.cost_to_go(m.double(), m.double(), m.double())
    # the planner methods pass the same refusals through
    with pytest.raises(RuntimeError, match="HIP device"):
        DifferentiableAstar().cost_to_go(m, m, m)
    with pytest.raises(RuntimeError, match="HIP device"):
        VanillaAstar().cost_to_go(m, m)
    with pytest.raises(NotImplementedError, match="16384"):
        VanillaAstar().cost_to_go(big, big)
    assert callable(NeuralAstar.cost_to_go)


def test_from_maps_needs_a_device_and_fields_to_dataset_follows_the_file_convention():
    from neural_astar.utils.data import DeviceMazeBatches, fields_to_dataset
    P = syn.maze_maps(3, 32, seed=2)
    with pytest.raises(RuntimeError, match="HIP device"):
        DeviceMazeBatches.from_maps(P.map_designs, P.goal_maps, "cpu")
    ok = P.map_designs[:, 0] > 0
    bfs = syn.geodesic_distance(ok, P.goal_maps.reshape(3, -1).argmax(1))
    d, pol, _ = FO.fields(P.map_designs, P.goal_maps, P.map_designs)
    od, op = fields_to_dataset(torch.from_numpy(d)[:, None], torch.from_numpy(pol))
    want = np.where(bfs >= 0, -bfs.astype(f32), -(bfs.max((1, 2), keepdims=True) + 1.0)).astype(f32)
    assert np.array_equal(od.numpy(), want[:, None]) and np.array_equal(op.numpy(), syn.optimal_policies(ok, bfs))
