"""CPU: ordered routes from the search launch (include/nastar_routes.h, ``plan_routes()``) -- everything that needs no GPU.

1. the numpy route oracle (tests/route_oracle.py) is pinned by the reference's own ``paths`` masks: every search golden of 32x32 or less,
   four named ones, and the neighbor_filter / heuristic vectors through their loaders;
2. the second header against ``_native.ROUTE_SIGNATURES`` and ``ops.route_forward_calls``; the library exports its three symbols;
3. the argument refusals of both entry points (made before any HIP call, so they need no device);
4. the Python surface: ``plan_routes`` on the three classes, its refusals before the library is touched, ``route_coords``.
"""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import golden_util as G
import heuristic_oracle as HO
import neighbor_golden as NG
import route_oracle as RO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMED = ["rand20x45_ucost_g050", "grad_rand7x5_eval_g050", "maze32_train_T005", "maze32_train_T025"]
SMALL = sorted(set([n for n in G.names() if max(G.load(n).H, G.load(n).W) <= 32] + NAMED))
MAX_CELLS = 6400  # the numpy oracle on the neighbor_filter / heuristic vectors: up to 80x80 (the GPU tests' largest case from these sets)


def coupling_possible(g_ratio):
    return not (0.5 <= float(g_ratio) < 1.0)


def check_routes(r, paths, start_maps, goal_maps, passable, W, mask):
    """the properties of the issue's item 1, for every map of a golden"""
    moves = set(HO.offsets(mask))
    B = paths.shape[0]
    for b in range(B):
        cells = r.routes[b]
        on = np.flatnonzero(paths[b].reshape(-1)).tolist()
        start, goal = int(start_maps[b].reshape(-1).argmax()), int(goal_maps[b].reshape(-1).argmax())
        assert sorted(cells) == on, f"map {b}: the route's cells are not the cells of the golden paths mask"
        assert len(set(cells)) == len(cells), f"map {b}: a cell repeats"
        assert cells[-1] == goal, f"map {b}: the goal is not last"
        assert r.lengths[b] == len(cells) == int(paths[b].sum())
        ok = passable[b].reshape(-1) != 0
        for a, c in zip(cells, cells[1:]):
            assert (c // W - a // W, c % W - a % W) in moves, f"map {b}: {a} -> {c} is not an allowed move"
            assert ok[c], f"map {b}: cell {c} is not passable"
        if r.reached[b]:
            assert cells[0] == start, f"map {b}: the search reached the goal but the route does not begin at the start"


@pytest.mark.parametrize("name", SMALL)
def test_oracle_routes_are_the_golden_paths_in_order(name):
    g = G.load(name)
    r = RO.plan(g.cost_maps, g.start_maps, g.goal_maps, g.passable, g.g_ratio, g.max_iters, lockstep=g.B > 1 and coupling_possible(g.g_ratio))
    assert np.array_equal(r.paths, g.paths[:, 0]) and np.array_equal(r.histories, g.histories[:, 0])
    check_routes(r, g.paths[:, 0], g.start_maps, g.goal_maps, g.passable, g.W, HO.MOORE8)
    if name == "maze32_train_T005":  # the "goal never opened" case: the budget ends first on nearly every map, and the route is [goal]
        never = ~r.reached
        assert never[:6].all() and never.sum() >= 24 and (r.lengths[never] == 1).all()


def test_the_small_set_holds_the_cases_the_gpu_tests_use():
    assert {"maze32_vanilla_g050", "maze32_train_T005", "maze32_train_T025", "rand20x45_ucost_g050", "grad_rand7x5_eval_g050", "rand32_ucost_g050",
            "grad_rand16_eval_g080", "maze32_cnncost_g050"} <= set(SMALL)


@pytest.mark.parametrize("name", [n for n in NG.names() if np.prod(NG.load(n).map_designs.shape[-2:]) <= MAX_CELLS])
def test_oracle_routes_on_the_neighbor_filter_vectors(name):
    g = NG.load(name)
    B, _, H, W = g.map_designs.shape
    mask = NG.mask_of(g.filter)
    r = RO.plan(g.cost_maps, g.start_maps, g.goal_maps, g.map_designs, g.g_ratio, g.max_iters, mask, lockstep=B > 1 and coupling_possible(g.g_ratio))
    assert np.array_equal(r.paths, g.paths[:, 0]) and np.array_equal(r.histories, g.histories[:, 0])
    check_routes(r, g.paths[:, 0], g.start_maps, g.goal_maps, g.map_designs, W, mask)


@pytest.mark.parametrize("name", [n for n in HO.names() if np.prod(HO.load(n).map_designs.shape[-2:]) <= MAX_CELLS])
def test_oracle_routes_on_the_heuristic_vectors(name):
    g = HO.load(name)
    B, _, H, W = g.map_designs.shape
    r = RO.plan(g.cost_maps, g.start_maps, g.goal_maps, g.map_designs, g.g_ratio, g.max_iters, g.mask, h0=g.h0, lockstep=B > 1)
    assert np.array_equal(r.paths, g.paths[:, 0]) and np.array_equal(r.histories, g.histories[:, 0])
    check_routes(r, g.paths[:, 0], g.start_maps, g.goal_maps, g.map_designs, W, g.mask)


def test_rows_keep_the_last_cells_and_pad_with_minus_one():
    r = RO.Routes([[5, 6, 7, 8], [], [3]], np.array([4, 0, 1], np.int32), np.zeros(3), None, None, None, None)
    assert RO.rows(r, 6).tolist() == [[5, 6, 7, 8, -1, -1], [-1] * 6, [3, -1, -1, -1, -1, -1]]
    assert RO.rows(r, 2).tolist() == [[7, 8], [-1, -1], [3, -1]]


# ---- 2. header and binding -----------------------------------------------------------------------------------------------------------
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


def test_second_header_and_route_signatures_agree():
    from neural_astar import _native
    protos = _prototypes("nastar_routes.h")
    assert sorted(protos) == sorted(_native.ROUTE_SIGNATURES) == ["nastar_forward_routes", "nastar_forward_routes_batchloop_finish", "nastar_routes_abi"]
    for name, (ret, args) in protos.items():
        assert ret == "i", name
        assert _native.ROUTE_SIGNATURES[name] == ret + " " + "".join(k for k, _ in args), name
    assert not set(_native.ROUTE_SIGNATURES) & set(_native.SIGNATURES)  # a table of its own: SIGNATURES stays include/nastar.h
    # the two entry points take the parameters of their _heuristic twins in nastar.h, in that order, and the four route outputs before the stream
    base = _prototypes("nastar.h")
    group = [("p", "routes_out"), ("i", "route_cap"), ("p", "route_len_out"), ("p", "route_cost_out")]
    for new, old in (("nastar_forward_routes", "nastar_forward_ex_heuristic"),
                     ("nastar_forward_routes_batchloop_finish", "nastar_forward_batchloop_finish_heuristic")):
        assert protos[new][1] == base[old][1][:-1] + group + [("p", "stream")], new
    hdr = open(os.path.join(ROOT, "include", "nastar_routes.h")).read()
    assert re.search(r"^#define NASTAR_ROUTES_ABI 1\b", hdr, flags=re.M) and not re.search(r"#define NASTAR_VERSION", hdr)


def test_library_exports_the_route_symbols():
    from neural_astar import _native
    lib = _native.load()
    for sym in _native.ROUTE_SIGNATURES:
        assert hasattr(lib, sym), sym
    assert lib.nastar_routes_abi() == 1
    assert lib.nastar_forward_routes.argtypes is not None and len(lib.nastar_forward_routes.argtypes) == 29


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("mask,with_h0", [(None, False), (0x0AA, False), (None, True), (0x0AA, True)])
def test_assembled_route_calls_put_every_value_under_its_header_name(mask, with_h0, exact):
    from neural_astar import ops
    protos = _prototypes("nastar_routes.h")
    header = [n for _, n in protos["nastar_forward_routes"][1]]
    assert list(inspect.signature(ops.route_forward_calls).parameters) == [n for n in header if n != "packed_out"] + ["exact"]
    v = {}

    def s(name):
        return v.setdefault(name, 0x1000 + 0x10 * len(v))

    for with_cost, with_summary, with_counter, with_order in [(a, b, c, d) for a in (0, 1) for b in (0, 1) for c in (0, 1) for d in (0, 1)]:
        given = {"cost": s("cost"), "start": s("start"), "goal": s("goal"), "passable": s("passable"), "B": 7, "H": 32, "W": 48, "g_ratio": 0.25,
                 "max_iters": 99, "histories_out": s("histories_out"), "paths_out": s("paths_out"), "sel_log_out": None, "iters_out": s("iters_out"),
                 "status_out": s("status_out"), "workspace": s("workspace") if exact else None, "workspace_bytes": 4096 if exact else 0,
                 "flags": ops.FLAG_MARK_COUPLED if exact else 0, "order": s("order") if with_order else None, "order_out": None,
                 "status_summary": s("status_summary") if with_summary else 0, "completion_counter": s("completion_counter") if with_counter else 0,
                 "neighbor_mask": mask, "h0": s("h0") if with_h0 else None, "routes_out": s("routes_out"), "route_cap": 33,
                 "route_len_out": s("route_len_out"), "route_cost_out": s("route_cost_out") if with_cost else None, "stream": s("stream")}
        launch, finish = ops.route_forward_calls(**given, exact=exact)
        assert ops.route_forward_calls(*given.values(), exact) == (launch, finish)
        expect = dict(given, packed_out=None, neighbor_mask=ops.NEIGHBORS_MOORE8 if mask is None else mask,
                      status_summary=given["status_summary"] or None,
                      completion_counter=(given["completion_counter"] or None) if with_summary else None)
        calls = [(launch, "nastar_forward_routes")] + ([(finish, "nastar_forward_routes_batchloop_finish")] if exact else [])
        assert exact or finish is None
        for (name, args), want in calls:
            assert name == want
            params = [n for _, n in protos[name][1]]
            assert len(args) == len(params) and params[-1] == "stream"
            for prm, val in zip(params, args):
                assert val == expect[prm] and type(val) is type(expect[prm]), (name, prm, val, expect[prm])


# ---- 3. refusals, made before any HIP call ---------------------------------------------------------------------------------------------
def _route_args(**over):
    p = 0x10000  # never dereferenced: every call below is refused on its arguments
    a = dict(cost=p, start=p, goal=p, passable=p, B=2, H=8, W=8, g_ratio=0.5, max_iters=64, histories_out=p, paths_out=p, sel_log_out=None,
             iters_out=p, status_out=p, packed_out=None, workspace=None, workspace_bytes=0, flags=0, order=None, order_out=None,
             status_summary=None, completion_counter=None, neighbor_mask=0x1EF, h0=None, routes_out=p, route_cap=64, route_len_out=p,
             route_cost_out=None, stream=None)
    a.update(over)
    return a


@pytest.mark.parametrize("over,rc", [(dict(routes_out=None), 5), (dict(route_len_out=None), 5), (dict(route_cap=0), 1), (dict(route_cap=-3), 1),
                                     (dict(neighbor_mask=0x1FF), 2), (dict(neighbor_mask=0x200), 2), (dict(flags=1 << 20), 2),
                                     (dict(cost=None), 5), (dict(B=0), 1)])
def test_forward_routes_refuses_bad_arguments_without_a_device(over, rc):
    from neural_astar import _native
    assert _native.load().nastar_forward_routes(*_route_args(**over).values()) == rc


@pytest.mark.parametrize("over,rc", [(dict(routes_out=None), 5), (dict(route_len_out=None), 5), (dict(route_cap=0), 1),
                                     (dict(neighbor_mask=0x010), 2), (dict(workspace=None), 5), (dict(max_iters=0), 1)])
def test_forward_routes_batchloop_finish_refuses_bad_arguments_without_a_device(over, rc):
    from neural_astar import _native
    a = _route_args(workspace=0x10000, workspace_bytes=1 << 20)
    a.update(over)
    for k in ("packed_out", "flags", "order", "order_out", "status_summary", "completion_counter"):
        a.pop(k)
    assert _native.load().nastar_forward_routes_batchloop_finish(*a.values()) == rc


# ---- 4. the Python surface ---------------------------------------------------------------------------------------------------------------
def test_plan_routes_exists_on_the_three_classes():
    from neural_astar.planner import NeuralAstar, VanillaAstar
    from neural_astar.planner.differentiable_astar import DifferentiableAstar, RoutedAstarOutput
    assert list(inspect.signature(DifferentiableAstar.plan_routes).parameters) == ["self", "cost_maps", "start_maps", "goal_maps", "obstacles_maps",
                                                                                 "heuristic_maps", "max_route_len"]
    for cls in (VanillaAstar, NeuralAstar):
        assert list(inspect.signature(cls.plan_routes).parameters) == ["self", "map_designs", "start_maps", "goal_maps", "heuristic_maps", "max_route_len"]
    assert NeuralAstar.plan_routes is not VanillaAstar.plan_routes
    assert RoutedAstarOutput._fields == ("histories", "paths", "routes", "route_lengths", "route_costs")
    assert "detached" in DifferentiableAstar.plan_routes.__doc__


def _tiny():
    m = torch.ones(2, 1, 8, 8)
    s = torch.zeros(2, 1, 8, 8)
    g = torch.zeros(2, 1, 8, 8)
    s[:, 0, 0, 0] = 1
    g[:, 0, 7, 7] = 1
    return m, s, g


def _planners():
    from neural_astar.planner import NeuralAstar, VanillaAstar
    from neural_astar.planner.differentiable_astar import DifferentiableAstar
    da = DifferentiableAstar()
    return [("DifferentiableAstar", lambda m, s, g, **k: da.plan_routes(m, s, g, m, **k)),
            ("VanillaAstar", VanillaAstar().plan_routes), ("NeuralAstar", NeuralAstar(encoder_depth=1).eval().plan_routes)]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_plan_routes_refuses_before_the_library_is_reached(which, monkeypatch):
    from neural_astar import _native

    def no_load():
        raise AssertionError("_native.load() was reached")

    monkeypatch.setattr(_native, "load", no_load)
    name, plan = _planners()[which]
    m, s, g = _tiny()
    for bad in (0, -1, 2.5, True, "8"):
        with pytest.raises(ValueError, match="max_route_len"):
            plan(m, s, g, max_route_len=bad)
    with pytest.raises(ValueError, match="heuristic_maps"):
        plan(m, s, g, heuristic_maps=torch.zeros(2, 1, 8, 7))
    with pytest.raises(TypeError, match="heuristic_maps"):
        plan(m, s, g, heuristic_maps=torch.zeros(2, 1, 8, 8, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU"):  # CPU tensors: the package's error, not a launch
        plan(m, s, g)
    with pytest.raises(RuntimeError, match="no CPU"):
        plan(m, s, g, heuristic_maps=torch.zeros(2, 1, 8, 8), max_route_len=4)


def test_search_routes_refuses_a_bad_capacity_and_cpu_tensors():
    from neural_astar import ops
    m, s, g = _tiny()
    with pytest.raises(ValueError, match="route_cap"):
        ops.search_routes(m, s, g, m, 0.5, 64, route_cap=0)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.search_routes(m, s, g, m, 0.5, 64)


def test_route_coords_on_a_hand_made_tensor():
    from neural_astar.planner.differentiable_astar import route_coords
    routes = torch.tensor([[0, 6, 12, 13, -1], [9, -1, -1, -1, -1]], dtype=torch.int32)
    rc = route_coords(routes, 5)
    assert rc.shape == (2, 5, 2)
    assert rc[0].tolist() == [[0, 0], [1, 1], [2, 2], [2, 3], [-1, -1]]
    assert rc[1].tolist() == [[1, 4], [-1, -1], [-1, -1], [-1, -1], [-1, -1]]
