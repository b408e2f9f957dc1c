"""GPU tests (-m gpu) of the large-map search at the seams of its two-level open list (csrc/nastar_search_hybrid.hip.h,
csrc/nastar_forward_hybrid_body.inc): the scenarios of tests/hybrid_edges.py -- whose reach tests/test_hybrid_edges.py shows on the CPU --
through the kernels, bit for bit against the CPU oracle: histories, paths, step counts, statuses and selection logs.

Scenarios of one shape, g_ratio and budget run as ONE batch of distinct maps, in two orders, so that every scenario is searched at a batch
index other than 0 (the slab offset b * slab_bytes, the per-map reset of the open list in LDS); a scenario that is alone in its class is
paired with itself searched the other way round (``name~``).  The spl 2, spl 5 and padded-tail scenarios also go through the masked, the
heuristic and the multi-source kernel and through the routed launch; the lock-step batch through the batch-loop finish.  Every comparison
is an equality.  What costs time is the oracle, which scans every cell per step: at most four of its runs per test.
"""
import functools

import numpy as np
import pytest
import torch

import hybrid_edges as E

pytestmark = pytest.mark.gpu

GUARD = 8192  # bytes in front of and behind every carved output
SENTINEL = 0xA5


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


@functools.lru_cache(maxsize=None)
def _steps_of(name):
    return int(_oracle(name).iters[0])


@functools.lru_cache(maxsize=None)
def _oracle(name, mask=None, mode="sm"):
    """the CPU oracle's outputs for scenario `name` (one map, or the lock-step batch): computed once, shared, never modified.  Start / goal
    maps that are not one-hot go in as the one-hot of their highest cell -- the kernels' contract."""
    from oracle import oracle as O
    sc = E.build(name, _steps_of)
    o = O.forward(sc.cost, E.last_onehot(sc.start), E.last_onehot(sc.goal), sc.passable, sc.g_ratio, sc.max_iters, mode=mode, want_log=True,
                  **({} if mask is None else {"neighbor_mask": mask}))
    for a in (o.histories, o.paths, o.iters, o.sel_log):
        a.setflags(write=False)
    return o


def _batch(names):
    """the scenarios `names` as one batch -> (cost, start, goal, passable [B,H,W], g_ratio, max_iters)"""
    scs = [E.build(n, _steps_of) for n in names]
    assert len({(s.cost.shape, s.g_ratio, s.max_iters) for s in scs}) == 1 and all(s.cost.shape[0] == 1 for s in scs), names
    return tuple(np.concatenate([s[k] for s in scs]) for k in range(1, 5)) + (scs[0].g_ratio, scs[0].max_iters)


def _check(out, refs, what, status=True):
    """kernel outputs (hist, paths, iters, status, log) of a batch against one oracle output per map, bit for bit"""
    hist, paths, iters, st, log = (x.cpu().numpy() for x in out[:5])
    for b, o in enumerate(refs):
        n = int(o.iters[0])
        assert int(iters[b]) == n, f"{what}[{b}]: {int(iters[b])} steps, the oracle {n}"
        assert not status or int(st[b]) == int(o.map_status[0]), f"{what}[{b}]: status {int(st[b])}, the oracle {int(o.map_status[0])}"
        diff = np.flatnonzero(log[b, :n] != o.sel_log[0, :n])
        assert diff.size == 0, f"{what}[{b}]: selection logs differ first at step {diff[0]}: {log[b, diff[0]]} != {o.sel_log[0, diff[0]]}"
        assert np.array_equal(hist[b].view(np.uint32), o.histories[0].view(np.uint32)), f"{what}[{b}]: histories"
        if int(o.map_status[0]) == 0:  # (a map without a route has no path: the reference raises there)
            assert np.array_equal(paths[b], o.paths[0]), f"{what}[{b}]: paths"


def _search(batch, **kw):
    from neural_astar import ops
    cost, start, goal, passable, g_ratio, max_iters = batch
    assert ops.workspace_bytes(cost.shape) > 0, f"{cost.shape}: not a large-map size any more"
    out = ops.search_nograd(_t(cost), _t(start), _t(goal), _t(passable), g_ratio, max_iters, want_log=True, **kw)
    torch.cuda.synchronize()
    return out


# ---- every scenario, batched by (shape, g_ratio, budget) -----------------------------------------------------------------------------------
def _groups():
    g = []
    for H, W in E.LADDER_SHAPES:
        spl = E.geometry(H, W)[3]
        g.append((f"spl{spl}_{H}x{W}_tie", f"spl{spl}_{H}x{W}_tie~"))
        if (H, W) == (513, 512):
            g.append(("spl2_513x512_rnd", "multihot_near", "multihot_far", "wall_513x512"))
        else:
            g.append((f"spl{spl}_{H}x{W}_rnd", f"spl{spl}_{H}x{W}_rnd~"))
    g.append(("spl5_1024x1152_rnd_g0", "spl5_1024x1152_rnd_g0~"))
    g += [(f"thin_{H}x{W}_far", f"thin_{H}x{W}_near") for H, W in E.THIN_SHAPES]
    g += [(f"pad_{H}x{W}_{k}", f"pad_{H}x{W}_{k}_swap") for H, W in E.PAD_SHAPES for k in ("rnd", "tie")]
    g += [(f"budget_{b}", f"budget_{b}~") for b in E.BUDGETS]
    return g


GROUPS = _groups()


def test_every_scenario_of_the_table_is_in_a_group():
    named = {n for g in GROUPS for n in g}
    assert {n for n, r in E.table().items() if not r.lock} | {f"budget_{b}" for b in E.BUDGETS} <= named


@pytest.mark.parametrize("names", GROUPS, ids=lambda g: "+".join(g))
def test_scenarios_equal_the_oracle_at_every_batch_index(names):
    refs = [_oracle(n) for n in names]
    for order in (list(range(len(names))), list(range(len(names)))[::-1]):
        picked = [names[i] for i in order]
        _check(_search(_batch(picked)), [refs[i] for i in order], "+".join(picked))


# ---- the other kernel families --------------------------------------------------------------------------------------------------------------
FAMILY_ROWS = ["spl2_513x512_tie", "spl2_513x512_rnd", "spl2_512x514_tie", "spl2_512x514_rnd", "spl5_1024x1152_tie", "spl5_1024x1152_rnd"] + \
              [n for n in E.table() if n.startswith("pad_")]


def _twice(name):
    """the scenario as a batch of two: the second copy is searched behind a slab offset"""
    return _batch([name, name])


@pytest.mark.parametrize("name", FAMILY_ROWS)
def test_masked_and_heuristic_kernels_at_the_seams(name):
    """Moore-8 passed explicitly (the masked kernel) and the built-in heuristic passed as a tensor (the heuristic kernel) give the plain
    call's bits; the von Neumann neighbourhood equals the oracle's masked state machine"""
    from neural_astar import ops
    batch = _twice(name)
    o = _oracle(name)
    plain = _search(batch)
    _check(plain, [o, o], name)
    for what, kw in (("masked Moore-8", {"neighbor_mask": ops.NEIGHBORS_MOORE8}), ("heuristic", {"heuristic": ops.heuristic(_t(batch[2]))})):
        out = _search(batch, **kw)
        _check(out, [o, o], f"{name} {what}")
        assert all(torch.equal(a, b) for a, b in zip(out[:4], plain[:4])), f"{name} {what}: not the plain call's bits"
    ov = _oracle(name, ops.NEIGHBORS_VON_NEUMANN)
    _check(_search(batch, neighbor_mask=ops.NEIGHBORS_VON_NEUMANN), [ov, ov], f"{name} von Neumann")


def _three_sources(sc):
    """the start, its neighbour in the same chunk, and a cell on the far side of the seam the scenario is built around (another super-chunk
    and owner lane; padded-tail maps have one super-chunk: three rows up, another chunk)"""
    _, H, W = sc.cost.shape
    s = int(np.flatnonzero(sc.start)[0])
    near = s + 1 if (s + 1) >> 6 == s >> 6 and s + 1 < H * W else s - 1
    if sc.name.startswith("pad_"):
        far = s - 3 * W
    else:
        r, c = E.seam(H, W)
        far = (r + 1) * W + c + 2
        assert far >> 12 != s >> 12 and (far >> 12) // E.geometry(H, W)[3] != (s >> 12) // E.geometry(H, W)[3]
    assert near >> 6 == s >> 6 and far >> 6 != s >> 6
    m = sc.start.copy()
    m.reshape(-1)[[near, far]] = 1.0
    return m


@pytest.mark.parametrize("name", FAMILY_ROWS)
def test_sources_kernel_at_the_seams(name):
    """multi_source with the one-hot start is the plain search; with three sources it equals the numpy multi-source oracle (81x81 and 83x79, with a
    cell count that is no multiple of 4, read their start maps cell by cell, the other shapes 16 bytes at a time)"""
    import multisource_oracle as MO
    sc = E.build(name, _steps_of)
    o = _oracle(name)
    _check(_search(_twice(name), multi_source=True), [o, o], f"{name} one source")
    start3 = _three_sources(sc)
    r = MO.search(sc.cost, start3, sc.goal, sc.passable, None, sc.g_ratio, sc.max_iters)
    cost, _, goal, passable, g_ratio, max_iters = _twice(name)
    hist, paths, iters, status, log = (x.cpu().numpy() for x in _search((cost, np.concatenate([start3, start3]), goal, passable, g_ratio, max_iters),
                                                                       multi_source=True))
    n = int(r.iters[0])
    for b in range(2):
        assert int(iters[b]) == n and int(status[b]) == int(r.status[0]), f"{name}[{b}]: {int(iters[b])} steps, status {int(status[b])}"
        assert np.array_equal(log[b, :n], np.asarray(r.sel[0], np.int32)), f"{name}[{b}]: selection log"
        assert np.array_equal(hist[b].view(np.uint32), r.histories[0].view(np.uint32)) and np.array_equal(paths[b], r.paths[0]), f"{name}[{b}]"


@pytest.mark.parametrize("name", ["spl5_1024x1152_tie", "spl5_1024x1152_rnd"] + [n for n in E.table() if n.startswith("pad_")])
def test_routes_at_the_seams(name):
    """ops.search_routes against tests/route_oracle.py: the ordered route, its length, and its cost -- the fp64 sum of the costs of the route
    cells but the goal, added up from the goal's parent backwards as the walk meets them, rounded once"""
    import route_oracle as RO
    from neural_astar import ops
    sc = E.build(name, _steps_of)
    cost, start, goal, passable, g_ratio, max_iters = _twice(name)
    assert ops.workspace_bytes(cost.shape) > 0
    out = ops.search_routes(_t(cost), _t(start), _t(goal), _t(passable), g_ratio, max_iters)
    torch.cuda.synchronize()
    r = RO.plan(sc.cost, sc.start, sc.goal, sc.passable, g_ratio, max_iters)
    o = _oracle(name)
    routes, lengths, costs = (x.cpu().numpy() for x in out[5:8])
    want = RO.rows(r, routes.shape[1])[0]
    total = 0.0
    for c in r.routes[0][-2::-1]:
        total += float(sc.cost.reshape(-1)[c])
    for b in range(2):
        assert np.array_equal(out[0][b].cpu().numpy(), o.histories[0]) and np.array_equal(out[1][b].cpu().numpy(), o.paths[0]), f"{name}[{b}]"
        assert int(lengths[b]) == int(r.lengths[0]) and np.array_equal(routes[b], want), f"{name}[{b}]: route"
        assert costs[b].view(np.uint32) == np.float32(total).view(np.uint32), f"{name}[{b}]: route cost {costs[b]!r} != {np.float32(total)!r}"


# ---- lock-step: the batch-loop finish with the goal held open on a super-chunk border ------------------------------------------------------
@pytest.mark.parametrize("name", [n for n, r in E.table().items() if r.lock])
@pytest.mark.parametrize("flip", [False, True])
def test_lock_step_batch_equals_the_literal_batch_loop(name, flip):
    """exact=True: map 0 (batch-coupled) is re-run in lock-step mode up to the step at which both maps select their goal -- histories and
    paths of the oracle's literal batch loop, its log over all t_batch + 1 steps; map 1 (a fixed point) keeps its own search.  The plain call
    equals the state machine.  `flip`: the coupled map at batch index 1."""
    sc = E.build(name)
    od, osm = _oracle(name, None, "dense"), _oracle(name)
    order = [1, 0] if flip else [0, 1]
    batch = tuple(a[order] for a in sc[1:5]) + (sc.g_ratio, sc.max_iters)
    hist, paths, iters, status, log = (x.cpu().numpy() for x in _search(batch))
    for i, b in enumerate(order):
        n = int(osm.iters[b])
        assert int(iters[i]) == n and int(status[i]) == 0 and np.array_equal(log[i, :n], osm.sel_log[b, :n]), f"{name} plain, map {b}"
        assert np.array_equal(hist[i], osm.histories[b]) and np.array_equal(paths[i], osm.paths[b]), f"{name} plain, map {b}"
    hist, paths, iters, status, log = (x.cpu().numpy() for x in _search(batch, exact=True))
    assert not np.array_equal(od.histories[0], osm.histories[0])  # (map 0 is in the coupled class: the finish has work to do)
    for i, b in enumerate(order):
        n = od.t_batch + 1 if b == 0 else int(od.iters[b])  # the re-run map reports the batch's steps, the other its own
        assert int(iters[i]) == n and int(status[i]) == 0, f"{name} exact, map {b}: {int(iters[i])} steps, {n} expected"
        assert np.array_equal(hist[i], od.histories[b]) and np.array_equal(paths[i], od.paths[b]), f"{name} exact, map {b}"
        assert np.array_equal(log[i, :n], od.sel_log[b, :n]), f"{name} exact, map {b}: selection log"
    assert int(iters.max()) - 1 == od.t_batch


# ---- guard bytes around every output of the padded-tail maps -------------------------------------------------------------------------------
@pytest.mark.parametrize("names", [g for g in GROUPS if g[0].startswith("pad_")], ids=lambda g: "+".join(g))
def test_guard_bytes_around_the_outputs_of_padded_maps_stay_untouched(names):
    """the C ABI on outputs carved out of sentinel-filled buffers: a store to a padded cell of the last chunk (cells HW .. 64 ceil(HW / 64))
    of the last map would land behind histories or paths, one of map 0 in map 1's rows -- which the comparison with the oracle sees"""
    from neural_astar import _native, ops
    lib = _native.load()
    dev = _dev()
    cost, start, goal, passable, g_ratio, max_iters = _batch(names)
    B, H, W = cost.shape
    c, s, g, p = (_t(x) for x in (cost, start, goal, passable))
    sizes = {"histories": B * H * W * 4, "paths": B * H * W * 8, "sel_log": B * max_iters * 4, "iters": B * 4, "status": B * 4}
    bufs = {k: torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.uint8, device=dev) for k, n in sizes.items()}
    ptr = {k: b.data_ptr() + GUARD for k, b in bufs.items()}
    ws_bytes = ops.workspace_bytes((B, H, W))
    assert ws_bytes > 0
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    (symbol, args), _ = ops.forward_calls(c.data_ptr(), s.data_ptr(), g.data_ptr(), p.data_ptr(), B, H, W, g_ratio, max_iters, ptr["histories"],
                                          ptr["paths"], ptr["sel_log"], ptr["iters"], ptr["status"], ws.data_ptr(), ws_bytes, 0, None, None, None,
                                          None, torch.cuda.current_stream().cuda_stream)
    assert getattr(lib, symbol)(*args) == 0
    torch.cuda.synchronize()
    raw = {k: b.cpu().numpy() for k, b in bufs.items()}
    for k, n in sizes.items():
        assert (raw[k][:GUARD] == SENTINEL).all(), f"bytes in FRONT of {k} were written"
        assert (raw[k][GUARD + n:] == SENTINEL).all(), f"bytes BEHIND {k} were written"
    take = lambda k, dt: np.frombuffer(raw[k][GUARD:GUARD + sizes[k]].tobytes(), dt)  # noqa: E731
    out = (take("histories", np.float32).reshape(B, H, W), take("paths", np.int64).reshape(B, H, W), take("iters", np.int32),
           take("status", np.int32), take("sel_log", np.int32).reshape(B, max_iters))
    _check([torch.from_numpy(x.copy()) for x in out], [_oracle(n) for n in names], "+".join(names) + " carved")
