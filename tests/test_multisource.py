"""CPU: the multi-source search (include/nastar_sources.h, ``multi_source = True`` on the planners) -- everything that needs no GPU.

1. the numpy restatement (tests/multisource_oracle.py) reproduces every reference vector of tests/golden/multisource/: histories, paths and
   the selection of every step; the properties each vector was built for hold on the file; the generator's seed-rejection cap holds;
2. the third header against ``_native.SOURCE_SIGNATURES`` and the assembled call tuples; the library exports its four symbols; the other two
   tables are disjoint from it and keep their symbols;
3. the argument refusals of the three entry points (made before any HIP call);
4. the Python surface: the ``multi_source`` attribute on the three planner classes.
"""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import multisource_oracle as MO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORWARD = ["coupled16_g020", "dense8_allstarts", "field20x45_k3", "heur24_k3", "large140x150_k3", "large96_k4", "signed12_reparent",
           "unit16_samechunk", "unit32_k4", "unit64_k8", "vn20_k3"]
GRAD = ["grad_coupled16_g020_k3", "grad_field20x45_eval_k4", "grad_h0only_24_k3", "grad_large120_k3", "grad_large96_k3", "grad_unit32_train_T025_k3"]


def test_the_vector_set_is_complete_and_small():
    assert MO.names() == sorted(FORWARD + GRAD)
    for n in MO.names():
        assert os.path.getsize(os.path.join(MO.DIR, n + ".npz")) < 256 * 1024, n


def _restate(g):
    B = g.map_designs.shape[0]
    return MO.search(g.cost_maps, g.start_maps, g.goal_maps, g.map_designs, g.h0, g.g_ratio, g.max_iters, g.mask, lockstep=B > 1, with_maps=True)


@pytest.mark.parametrize("name", FORWARD + GRAD)
def test_restatement_reproduces_the_reference(name):
    g = MO.load(name)
    B = g.map_designs.shape[0]
    assert (g.start_maps.reshape(B, -1).sum(1) >= 2).all(), "every map of a vector holds at least two start cells"
    o, _ = _restate(g)
    assert (o.status == 0).all()
    assert np.array_equal(o.histories, g.histories[:, 0]), "histories"
    assert np.array_equal(o.paths, g.paths[:, 0]), "paths"
    assert o.t_batch == g.t_batch
    for b in range(B):
        n = len(o.sel[b])
        assert o.sel[b] == g.sel_log[b, :n].tolist(), f"map {b}: selections"
        assert (g.sel_log[b, n:] == int(g.goal_maps[b].reshape(-1).argmax())).all()  # ... then the goal, until the batch's loop ends


@pytest.mark.parametrize("name", FORWARD + GRAD)
def test_seed_rejection_cap(name):
    g = MO.load(name)
    assert g.tried >= 1 and g.rejected * 10 <= g.tried, f"{name}: {g.rejected} of {g.tried} seeds rejected"


@pytest.mark.parametrize("name", FORWARD)
def test_every_path_ends_at_a_source_with_an_unset_parent(name):
    g = MO.load(name)
    o, maps = _restate(g)
    for b, m in enumerate(maps):
        route = m.route(max(len(m.sel) - 1, 0))
        assert sorted(route) == np.flatnonzero(o.paths[b].reshape(-1)).tolist()
        assert route[-1] == m.goal and m.parent[route[0]] == MO.UNSET and route[0] in m.sources


def test_dropping_all_starts_but_the_last_changes_the_answer():
    """what ``multi_source = False`` computes on these inputs (the highest-index start only) is NOT the reference's answer"""
    import heuristic_oracle as HO
    changed = 0
    for name in ("unit32_k4", "field20x45_k3", "vn20_k3"):
        g = MO.load(name)
        B = g.map_designs.shape[0]
        one = HO.search(g.cost_maps, g.start_maps, g.goal_maps, g.map_designs, MO.default_h0(g.goal_maps[:, 0]), g.g_ratio, g.max_iters, g.mask,
                        lockstep=False)
        changed += sum(not np.array_equal(one.histories[b], g.histories[b, 0]) for b in range(B))
    assert changed >= 3


def test_unit16_samechunk_holds_adjacent_starts_and_both_corners():
    g = MO.load("unit16_samechunk")
    B, _, H, W = g.map_designs.shape
    assert (H, W) == (16, 16) and np.array_equal(g.cost_maps, g.map_designs)
    for b in range(B):
        s = np.flatnonzero(g.start_maps[b].reshape(-1))
        assert 0 in s and H * W - 1 in s
        assert any(x + 1 == y and x // 16 == y // 16 for x, y in zip(s, s[1:])), "a start pair adjacent in one row: one 16-cell chunk"


def test_dense8_holds_the_all_starts_map_and_the_goal_among_the_starts():
    g = MO.load("dense8_allstarts")
    goal = g.goal_maps.reshape(2, -1).argmax(1)
    s0, s1 = (g.start_maps[b].reshape(-1) != 0 for b in range(2))
    want = g.map_designs[0].reshape(-1) != 0
    want[goal[0]] = False
    assert np.array_equal(s0, want)
    assert s1[goal[1]] and s1.sum() >= 3
    assert g.paths[1].sum() == 1 and g.histories[1].sum() == 1  # the goal is selected first: the route is [goal]


def test_signed12_holds_a_path_through_two_start_cells():
    g = MO.load("signed12_reparent")
    assert g.cost_maps.min() < 0
    both = (g.paths[:, 0].reshape(len(g.paths), -1) * (g.start_maps[:, 0].reshape(len(g.paths), -1) != 0)).sum(1)
    assert both.max() >= 2, "a re-parented start cell on a path"


def test_coupled16_holds_a_map_that_leaves_its_fixed_point():
    g = MO.load("coupled16_g020")
    assert g.g_ratio == 0.2 and g.alone_histories is not None
    B = g.map_designs.shape[0]
    differs = [b for b in range(B) if not np.array_equal(g.alone_histories[b], g.histories[b])]
    assert differs, "no map's in-batch histories differ from its run alone"
    alone = MO.search(g.cost_maps, g.start_maps, g.goal_maps, g.map_designs, None, g.g_ratio, g.max_iters, g.mask, lockstep=False)
    assert np.array_equal(alone.histories, g.alone_histories[:, 0]) and np.array_equal(alone.paths, g.alone_paths[:, 0])


def test_large96_spreads_its_starts_over_the_open_list_levels():
    g = MO.load("large96_k4")
    assert g.map_designs.shape[-2:] == (96, 96)
    for b in range(g.map_designs.shape[0]):
        s = np.flatnonzero(g.start_maps[b].reshape(-1))
        pairs = [(x, y) for i, x in enumerate(s) for y in s[i + 1:]]
        assert any(x >> 6 == y >> 6 for x, y in pairs), "two starts in one 64-cell chunk"
        assert any(x >> 12 == y >> 12 and x >> 6 != y >> 6 for x, y in pairs), "two starts in one super-chunk, different chunks"
        assert any(x >> 12 != y >> 12 for x, y in pairs), "starts in different super-chunks"


def test_vector_settings():
    assert MO.load("vn20_k3").mask == MO.VON_NEUMANN
    assert MO.load("heur24_k3").h0 is not None and MO.load("heur24_k3").h0.min() < 0
    assert MO.load("large140x150_k3").map_designs.shape[-2:] == (140, 150)
    g = MO.load("grad_unit32_train_T025_k3")
    assert g.training and g.Tmax == 0.25 and g.grad_cost is not None
    g = MO.load("grad_h0only_24_k3")
    assert g.h0_only and g.grad_cost is None and g.grad_h0 is not None
    assert MO.load("grad_large120_k3").map_designs.shape[-2:] == (120, 120)
    for n in GRAD:
        g = MO.load(n)
        assert all(np.isfinite(x).all() for x in (g.grad_cost, g.grad_h0) if x is not None)


# ---- 2. header and binding -----------------------------------------------------------------------------------------------------------
_SCALARS = {"int": "i", "unsigned": "u", "float": "f", "double": "d", "size_t": "z", "long long": "q"}
SYMBOLS = ["nastar_backward_replay_sources", "nastar_forward_sources", "nastar_forward_sources_batchloop_finish", "nastar_sources_abi"]


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


def test_third_header_and_source_signatures_agree():
    from neural_astar import _native
    protos = _prototypes("nastar_sources.h")
    assert sorted(protos) == sorted(_native.SOURCE_SIGNATURES) == SYMBOLS
    for name, (ret, args) in protos.items():
        assert ret == "i", name
        assert _native.SOURCE_SIGNATURES[name] == ret + " " + "".join(k for k, _ in args), name
    # the entry points take the argument lists the issue names, parameter for parameter
    routes, base = _prototypes("nastar_routes.h"), _prototypes("nastar.h")
    assert protos["nastar_forward_sources"][1] == routes["nastar_forward_routes"][1]
    assert protos["nastar_forward_sources_batchloop_finish"][1] == routes["nastar_forward_routes_batchloop_finish"][1]
    assert protos["nastar_backward_replay_sources"][1] == base["nastar_backward_replay_ordered_heuristic"][1]
    hdr = open(os.path.join(ROOT, "include", "nastar_sources.h")).read()
    assert re.search(r"^#define NASTAR_SOURCES_ABI 1\b", hdr, flags=re.M) and not re.search(r"#define NASTAR_VERSION", hdr)


def test_the_other_tables_are_disjoint_and_keep_their_symbols():
    from neural_astar import _native
    assert not set(_native.SOURCE_SIGNATURES) & (set(_native.SIGNATURES) | set(_native.ROUTE_SIGNATURES))
    assert sorted(_native.ROUTE_SIGNATURES) == ["nastar_forward_routes", "nastar_forward_routes_batchloop_finish", "nastar_routes_abi"]
    assert sorted(_prototypes("nastar.h")) == sorted(_native.SIGNATURES) and sorted(_prototypes("nastar_routes.h")) == sorted(_native.ROUTE_SIGNATURES)
    assert not any("sources" in s for s in _native.SIGNATURES) and _native.EXPORTED_SYMBOLS == tuple(_native.SIGNATURES)


def test_library_exports_the_source_symbols():
    from neural_astar import _native
    lib = _native.load()
    for sym in _native.SOURCE_SIGNATURES:
        assert hasattr(lib, sym), sym
    assert lib.nastar_sources_abi() == 1 and lib.nastar_version() == 800 and lib.nastar_routes_abi() == 1
    assert len(lib.nastar_forward_sources.argtypes) == 29 and len(lib.nastar_backward_replay_sources.argtypes) == 24


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("with_routes", [False, True])
@pytest.mark.parametrize("mask,with_h0", [(None, False), (0x0AA, False), (None, True), (0x0AA, True)])
def test_assembled_forward_calls_put_every_value_under_its_header_name(mask, with_h0, with_routes, exact):
    from neural_astar import ops
    protos = _prototypes("nastar_sources.h")
    header = [n for _, n in protos["nastar_forward_sources"][1]]
    assert list(inspect.signature(ops.source_forward_calls).parameters) == [n for n in header if n != "packed_out"] + ["exact"]
    v = {}

    def s(name):
        return v.setdefault(name, 0x1000 + 0x10 * len(v))

    given = {"cost": s("cost"), "start": s("start"), "goal": s("goal"), "passable": s("passable"), "B": 7, "H": 32, "W": 48, "g_ratio": 0.25,
             "max_iters": 99, "histories_out": s("histories_out"), "paths_out": s("paths_out"), "sel_log_out": s("sel_log_out"),
             "iters_out": s("iters_out"), "status_out": s("status_out"), "workspace": s("workspace") if exact else None,
             "workspace_bytes": 4096 if exact else 0, "flags": ops.FLAG_MARK_COUPLED if exact else 0, "order": None, "order_out": None,
             "status_summary": s("status_summary"), "completion_counter": s("completion_counter"), "neighbor_mask": mask,
             "h0": s("h0") if with_h0 else None, "routes_out": s("routes_out") if with_routes else None, "route_cap": 33 if with_routes else 0,
             "route_len_out": s("route_len_out") if with_routes else None, "route_cost_out": s("route_cost_out") if with_routes else None,
             "stream": s("stream")}
    launch, finish = ops.source_forward_calls(**given, exact=exact)
    expect = dict(given, packed_out=None, neighbor_mask=ops.NEIGHBORS_MOORE8 if mask is None else mask)
    calls = [(launch, "nastar_forward_sources")] + ([(finish, "nastar_forward_sources_batchloop_finish")] if exact else [])
    assert exact or finish is None
    for (name, args), want in calls:
        assert name == want
        params = [n for _, n in protos[name][1]]
        assert len(args) == len(params) and params[-1] == "stream"
        for prm, val in zip(params, args):
            assert val == expect[prm] and type(val) is type(expect[prm]), (name, prm, val, expect[prm])


@pytest.mark.parametrize("mask,with_h0,with_order", [(None, False, False), (0x0AA, True, True), (None, True, False)])
def test_assembled_replay_call_puts_every_value_under_its_header_name(mask, with_h0, with_order):
    from neural_astar import ops
    protos = _prototypes("nastar_sources.h")
    params = [n for _, n in protos["nastar_backward_replay_sources"][1]]
    given = dict(cost=0x10, start=0x20, goal=0x30, passable=0x40, sel_log=0x50, B=3, H=20, W=45, g_ratio=0.5, max_iters=2025, iters=0x60,
                 t_batch=0x70, grad_cost=0x80, workspace=0x90, ws_bytes=1 << 16, stream=0xA0, grad_hist=0xB0, flags=ops.FLAG_LOCKSTEP,
                 order=0xC0 if with_order else None, neighbor_mask=mask, heuristic=0xD0 if with_h0 else None)
    name, args = ops.replay_call(**given, multi_source=True)
    assert name == "nastar_backward_replay_sources" and len(args) == len(params)
    rename = dict(grad_histories="grad_hist", grad_loss_dev="grad_loss", t_batch_dev="t_batch", grad_cost_out="grad_cost", workspace_bytes="ws_bytes",
                  h0="heuristic")
    for prm, val in zip(params, args):
        want = given.get(rename.get(prm, prm))
        if prm == "neighbor_mask":
            want = ops.NEIGHBORS_MOORE8 if mask is None else mask
        assert val == want, (prm, val, want)
    # the one place that picks a family: the existing families are what they were
    assert ops._entry_family(None, None) == ("", ()) and ops._entry_family(0xAA, None) == ("_masked", (0xAA,))
    assert ops._entry_family(None, 5) == ("_heuristic", (ops.NEIGHBORS_MOORE8, 5)) and ops._entry_family(None, None, True) == ("_sources", (ops.NEIGHBORS_MOORE8, None))


# ---- 3. refusals, made before any HIP call ---------------------------------------------------------------------------------------------
def _fwd_args(**over):
    p = 0x10000  # never dereferenced: every call below is refused on its arguments
    a = dict(cost=p, start=p, goal=p, passable=p, B=2, H=8, W=8, g_ratio=0.5, max_iters=64, histories_out=p, paths_out=p, sel_log_out=None,
             iters_out=p, status_out=p, packed_out=None, workspace=None, workspace_bytes=0, flags=0, order=None, order_out=None,
             status_summary=None, completion_counter=None, neighbor_mask=0x1EF, h0=None, routes_out=None, route_cap=0, route_len_out=None,
             route_cost_out=None, stream=None)
    a.update(over)
    return a


@pytest.mark.parametrize("over,rc", [(dict(routes_out=0x10000), 5), (dict(routes_out=0x10000, route_len_out=0x10000, route_cap=0), 1),
                                     (dict(neighbor_mask=0x1FF), 2), (dict(neighbor_mask=0x010, cost=None), 2), (dict(flags=1 << 20), 2),
                                     (dict(cost=None), 5), (dict(B=0), 1), (dict(H=2000, W=2000), 2)])
def test_forward_sources_refuses_bad_arguments_without_a_device(over, rc):
    from neural_astar import _native
    assert _native.load().nastar_forward_sources(*_fwd_args(**over).values()) == rc


@pytest.mark.parametrize("over,rc", [(dict(routes_out=0x10000), 5), (dict(neighbor_mask=0x200), 2), (dict(workspace=None), 5), (dict(max_iters=0), 1),
                                     (dict(workspace_bytes=16), 6)])
def test_forward_sources_batchloop_finish_refuses_bad_arguments_without_a_device(over, rc):
    from neural_astar import _native
    a = _fwd_args(workspace=0x10000, workspace_bytes=1 << 20)
    a.update(over)
    for k in ("packed_out", "flags", "order", "order_out", "status_summary", "completion_counter"):
        a.pop(k)
    assert _native.load().nastar_forward_sources_batchloop_finish(*a.values()) == rc


def test_backward_replay_sources_refuses_bad_arguments_without_a_device():
    from neural_astar import _native
    lib, one, ws = _native.load(), 16, 1 << 20

    def bwd(gh=one, B=1, mask=0x1EF, h0=None, wsb=ws):
        return lib.nastar_backward_replay_sources(gh, None, None, None, one, one, one, one, one, B, 8, 8, 0.5, 64, one, None, one, one, wsb, 0, None, mask,
                                                  h0, None)

    assert bwd(mask=0x1FF, gh=None) == _native.NASTAR_ERR_UNSUPPORTED
    assert bwd(gh=None) == _native.NASTAR_ERR_NULL
    assert bwd(B=0) == _native.NASTAR_ERR_BAD_SHAPE
    assert bwd(wsb=16) == _native.NASTAR_ERR_WORKSPACE and bwd(wsb=16, h0=one) == _native.NASTAR_ERR_WORKSPACE


# ---- 4. the Python surface ---------------------------------------------------------------------------------------------------------------
def test_the_attribute_exists_on_the_three_classes_and_defaults_to_false():
    from neural_astar.planner import NeuralAstar, VanillaAstar
    from neural_astar.planner.differentiable_astar import DifferentiableAstar
    da = DifferentiableAstar()
    assert da.multi_source is False
    for planner in (VanillaAstar(), NeuralAstar(encoder_depth=1)):
        assert planner.multi_source is False and planner.astar.multi_source is False
        planner.multi_source = True  # forward() and plan_routes() of the wrapper search through self.astar
        assert planner.astar.multi_source is True and planner.multi_source is True
        import copy
        assert copy.deepcopy(planner).multi_source is True
    assert "multi_source" in DifferentiableAstar.forward.__doc__ and "highest flat index" in DifferentiableAstar.forward.__doc__
    assert "multi_source" in DifferentiableAstar.plan_routes.__doc__
    state = da.__getstate__()
    state.pop("multi_source")  # a planner pickled before the attribute existed
    old = DifferentiableAstar.__new__(DifferentiableAstar)
    old.__setstate__(state)
    assert old.multi_source is False


def test_the_low_level_calls_take_the_flag_and_default_to_false():
    from neural_astar import ops
    for fn in (ops.search_nograd, ops._launch_search, ops._replay):
        p = inspect.signature(fn).parameters
        assert p["multi_source"].default is False, fn.__name__
    for op in (ops.astar_forward, ops.astar_forward_ordered, ops.astar_backward_replay):
        assert "multi" not in str(op._schema)  # the custom ops keep their schemas: the flag travels through ops.astar_forward_sources


# ---- 5. the lanes that search from ONE start cell per map must not answer for a multi-source planner ---------------------------------------
def test_fused_l1_step_falls_back_to_the_planner_for_a_multi_source_planner(monkeypatch):
    """``fused_l1_step`` is what ``PlannerModule.training_step`` and ``utils.distributed`` train through; its fused node searches and replays
    from one start cell per map, so with ``multi_source`` set it must go through ``planner(...)`` + L1Loss, as it does for a neighbor_filter"""
    from neural_astar import ops
    from neural_astar.planner import VanillaAstar
    from neural_astar.planner.differentiable_astar import AstarOutput
    from neural_astar.utils import training

    def fused(*a, **k):
        raise AssertionError("the fused single-start node was reached")

    monkeypatch.setattr(ops, "astar_l1_loss", fused)
    x = torch.ones(2, 1, 8, 8)
    va = VanillaAstar()
    calls = []

    def forward(map_designs, start_maps, goal_maps, *a, **k):
        calls.append(va.astar.multi_source)
        return AstarOutput(torch.zeros_like(map_designs).requires_grad_(True), torch.zeros_like(map_designs), [])

    monkeypatch.setattr(va, "forward", forward)
    va.multi_source = True
    loss, out = training.fused_l1_step(va, x, x.clone(), x.clone(), x.clone())
    assert calls == [True] and float(loss.detach()) == 1.0 and loss.requires_grad
    va.multi_source = False  # ... and the default planner still takes the fused node
    with pytest.raises((AssertionError, RuntimeError), match="fused single-start node|no CPU"):
        training.fused_l1_step(va, x, x.clone(), x.clone(), x.clone())
    assert calls == [True]


def test_in_flight_planner_refuses_a_multi_source_planner_before_anything_is_launched():
    from neural_astar.parallel import InFlightPlanner
    from neural_astar.planner import NeuralAstar, VanillaAstar
    x = torch.ones(2, 1, 8, 8)
    for planner in (VanillaAstar(), NeuralAstar(encoder_depth=1).eval()):
        fly = InFlightPlanner(planner)
        planner.multi_source = True
        with pytest.raises(NotImplementedError, match="multi_source"):
            fly.submit(x, x.clone(), x.clone())
        with pytest.raises(NotImplementedError, match="multi_source"):
            fly.submit_search(x, x.clone(), x.clone(), x)
        planner.multi_source = False
        with pytest.raises(RuntimeError, match="HIP device|no CPU"):  # the default planner gets as far as the device check
            fly.submit(x, x.clone(), x.clone())


def test_the_validation_pair_hands_the_flag_to_its_vanilla_planner(monkeypatch):
    from neural_astar.planner import NeuralAstar, VanillaAstar
    from neural_astar.utils import metrics
    seen = []
    monkeypatch.setattr(VanillaAstar, "forward", lambda self, *a, **k: seen.append(self.multi_source) or "va")
    na = NeuralAstar(encoder_depth=1).train()  # (training mode: the two-launch branch)
    monkeypatch.setattr(na, "encode", lambda *a: torch.ones(2, 1, 8, 8))
    monkeypatch.setattr(na, "perform_astar", lambda *a, **k: "na")
    x = torch.ones(2, 1, 8, 8)
    for flag in (True, False):
        na.multi_source = flag
        assert metrics.plan_with_vanilla(na, x, x.clone(), x.clone()) == ("na", "va")
    assert seen == [True, False]
