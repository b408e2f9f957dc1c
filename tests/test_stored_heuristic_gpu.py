"""GPU tests (-m gpu) of the search stream that keeps the heuristic where the cost word was (csrc/nastar_search_asm5.hip.h).

A map takes that stream when the caller hands ONE binary tensor over as cost map and obstacle map (what VanillaAstar does): the kernel sees
it from the pointers and from the values it loads, per map, with no flag.  The yardstick therefore needs no switch: the SAME call with
``passable = cost.clone()`` has a distinct pointer and takes the general stream, and every output -- histories, paths, iters, status, packed
masks, summary, and where asked the selection log, the coupled marks and the routes -- must hold the same bits.  A subset is also compared
with the CPU oracle.  Every output buffer has guard bytes behind it.

Shapes: 16x16, 32x32 (one chunk minimum per lane) and 64x64 (four, the diving loop); B = 1, 3, 65 and 130 (less than one wavefront's worth of
workgroups up to more than two blocks of the ranked placement).  The maps of a batch are drawn from one bank per size (``_bank``) that mixes
bench-style mazes, 25 % random obstacles, starts and goals in corners and on edges, start == goal, adjacent goals, starts and goals on
obstacles, unsolvable maps, an all-ones map, and maps that hold ONE value other than 0.0 / 1.0 (0.5, 2.0, -0.0, -1.0, NaN) next to ordinary
ones: those must equal the general path's result like their neighbours.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 64  # elements behind every output
SIZES = (16, 32, 64)
BATCHES = (1, 3, 65, 130)
POISON = (0.5, 2.0, -0.0, -1.0, float("nan"))


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- the bank of single maps -----------------------------------------------------------------------------------------------------------
_BANKS = {}


def _bank(W):
    """[(map [W, W] float32, start cell, goal cell, name)] -- computed once per size, shared, never modified"""
    if W in _BANKS:
        return _BANKS[W]
    from neural_astar.utils import synthetic as syn
    rng = np.random.default_rng(1000 + W)
    cases = []

    def rand_map():
        return (rng.random((W, W)) > 0.25).astype(np.float32)

    def add(m, s, g, name):
        cases.append((np.ascontiguousarray(m, dtype=np.float32), int(s[0]) * W + int(s[1]), int(g[0]) * W + int(g[1]), name))

    def idx(flat):
        return divmod(int(flat), W)

    mz = syn.maze_maps(4, W, seed=100 + W)
    for b in range(4):
        add(mz.map_designs[b, 0], idx(mz.start_maps[b, 0].argmax()), idx(mz.goal_maps[b, 0].argmax()), f"maze{b}")
    ro = syn.random_obstacle_maps(6, W, W, 0.25, seed=200 + W)
    for b in range(6):
        add(ro.map_designs[b, 0], idx(ro.start_maps[b, 0].argmax()), idx(ro.goal_maps[b, 0].argmax()), f"rand{b}")
    # one value that is neither 0.0 nor 1.0, in a cell next to the start (so the general path reads it), between ordinary maps
    for k, v in enumerate(POISON):
        m = ro.map_designs[k, 0].copy()
        s = idx(ro.start_maps[k, 0].argmax())
        n = (min(max(s[0] + (1 if s[0] < W - 1 else -1), 0), W - 1), s[1])
        m[n] = v
        add(m, s, idx(ro.goal_maps[k, 0].argmax()), f"poison{v}")
        add(ro.map_designs[5 - k, 0], idx(ro.start_maps[5 - k, 0].argmax()), idx(ro.goal_maps[5 - k, 0].argmax()), f"beside{v}")
    # corners and edges, start and goal forced passable (the map may still be unsolvable: both paths then agree on that too)
    pts = [(0, 0), (0, W - 1), (W - 1, 0), (W - 1, W - 1), (0, W // 2), (W // 2, 0), (W - 1, W // 2 - 1), (W // 2 + 1, W - 1)]
    for k, p in enumerate(pts):
        q = pts[(k + 3) % 8]
        m = rand_map()
        m[p] = m[q] = 1
        add(m, p, q, f"edge{k}")
        m = np.ones((W, W), np.float32)
        m[1:-1:3, 1:-1:2] = 0
        add(m, q, p, f"edge{k}r")
    # start == goal (passable, and on an obstacle); the goal next to the start
    m = rand_map()
    m[3, 5] = 1
    add(m, (3, 5), (3, 5), "start_is_goal")
    m = rand_map()
    m[7, 2] = 0
    add(m, (7, 2), (7, 2), "start_is_goal_blocked")
    for k, d in enumerate(((0, 1), (-1, -1), (1, 0), (1, -1))):
        m = rand_map()
        m[5, 5] = m[5 + d[0], 5 + d[1]] = 1
        add(m, (5, 5), (5 + d[0], 5 + d[1]), f"adjacent{k}")
    # the start on an obstacle (the reference expands it all the same): inside, in a corner, walled in
    for k, s in enumerate(((W // 2, W // 2), (0, 0), (W - 1, 3))):
        m = rand_map()
        m[s] = 0
        m[W // 3, W - 2] = 1
        add(m, s, (W // 3, W - 2), f"start_blocked{k}")
    m = np.ones((W, W), np.float32)
    m[3:6, 3:6] = 0
    add(m, (4, 4), (W - 1, W - 1), "start_walled_in")
    # the goal on an obstacle; the goal walled in (the open list runs empty)
    m = rand_map()
    m[2, 2] = 1
    m[W - 3, W - 4] = 0
    add(m, (2, 2), (W - 3, W - 4), "goal_blocked")
    m = np.ones((W, W), np.float32)
    m[W - 3, :] = 0
    add(m, (0, 0), (W - 1, W - 1), "goal_walled_in")
    m = rand_map()
    m[0, 0] = m[W - 1, W - 1] = 1
    m[:, W // 2] = 0
    add(m, (0, 0), (W - 1, W - 1), "split_map")
    # all ones
    add(np.ones((W, W), np.float32), (0, 0), (W - 1, W - 1), "ones_diagonal")
    add(np.ones((W, W), np.float32), (W // 2, W // 2 - 1), (1, W - 2), "ones_inner")
    _BANKS[W] = cases
    return cases


def _batch(W, B, first=0):
    """B maps of the bank, from case `first` on (cyclic) -> (maps, starts, goals) [B, W, W] float32, names"""
    bank = _bank(W)
    m = np.empty((B, W, W), np.float32)
    s = np.zeros((B, W * W), np.float32)
    g = np.zeros((B, W * W), np.float32)
    names = []
    for b in range(B):
        mm, si, gi, name = bank[(first + b) % len(bank)]
        m[b] = mm
        s[b, si] = 1
        g[b, gi] = 1
        names.append(name)
    return m, s.reshape(B, W, W), g.reshape(B, W, W), names


def _binary(names):
    """maps of the batch whose values are all 0.0 or 1.0"""
    return np.array([not n.startswith("poison") for n in names])


# ---- one launch, every output guarded ---------------------------------------------------------------------------------------------------
class _Out:
    """a device buffer of n elements with GUARD sentinel elements behind it"""

    def __init__(self, n, dtype, fill):
        self.n = n
        self.fill = fill
        self.t = torch.full((n + GUARD,), fill, dtype=dtype, device=_dev())

    def ptr(self):
        return self.t.data_ptr()

    def take(self, what):
        a = self.t.cpu().numpy()
        tail = a[self.n:]
        assert (tail == self.fill).all(), f"{what}: the guard behind the output was written"
        return a[:self.n].copy()


def _launch(m, s, g, *, alias, which="ex", g_ratio=0.5, max_iters=None, log=False, marks=False, routes=False, levels=None):
    """one search of the batch through the C ABI; alias: passable IS the cost tensor (stored heuristic), else a clone of it (general stream).
    -> {name: numpy array} of everything the launch wrote"""
    from neural_astar import _native, ops
    lib = _native.load()
    B, H, W = m.shape
    HW = H * W
    max_iters = HW if max_iters is None else max_iters
    ct, st, gt = _t(m), _t(s), _t(g)
    pt = ct if alias else ct.clone()
    assert (pt.data_ptr() == ct.data_ptr()) == alias
    flags = ops.FLAG_MARK_COUPLED if marks else 0
    ws_bytes = int(lib.nastar_workspace_bytes(B, H, W, flags)) if marks else 0
    outs = {
        "histories": _Out(B * HW, torch.float32, -3.0),
        "paths": _Out(B * HW, torch.int64, -3),
        "iters": _Out(B, torch.int32, -3),
        "status": _Out(B, torch.int32, -3),
        "packed": _Out(B * 2 * ((HW + 7) // 8), torch.uint8, 0xA5),
        "summary": _Out(ops.SUMMARY_WORDS, torch.int32, 0),
    }
    if log:
        outs["sel_log"] = _Out(B * max_iters, torch.int32, -3)
    if marks:
        outs["workspace"] = _Out(ws_bytes, torch.uint8, 0)
    cap = HW
    if routes:
        outs["routes"] = _Out(B * cap, torch.int32, -3)
        outs["route_len"] = _Out(B, torch.int32, -3)
        outs["route_cost"] = _Out(B, torch.float32, -3.0)
    counter = torch.zeros(1 + GUARD, dtype=torch.int32, device=_dev())
    head = (ct.data_ptr(), st.data_ptr(), gt.data_ptr(), pt.data_ptr(), B, H, W, float(g_ratio), int(max_iters), outs["histories"].ptr(),
            outs["paths"].ptr(), outs["sel_log"].ptr() if log else None, outs["iters"].ptr(), outs["status"].ptr(), outs["packed"].ptr(),
            outs["workspace"].ptr() if marks and ws_bytes else None, ws_bytes, flags)
    tail = (outs["summary"].ptr(), counter.data_ptr())
    if which == "levels":
        assert not routes and not log
        rc = lib.nastar_forward_levels(*head, _t(levels).data_ptr(), *tail, _stream())
    elif routes:
        rc = lib.nastar_forward_routes(*head, None, None, *tail, ops.NEIGHBORS_MOORE8, None, outs["routes"].ptr(), cap, outs["route_len"].ptr(),
                                       outs["route_cost"].ptr(), _stream())
    else:
        rc = lib.nastar_forward_ex(*head, None, None, *tail, _stream())
    assert rc == 0, (which, rc, _native.load().nastar_last_error())
    torch.cuda.synchronize()
    assert (counter.cpu().numpy() == 0).all()  # (B completions bring the cell back to 0; nothing behind it was touched)
    return {k: o.take(k) for k, o in outs.items()}


def _same_bits(a, b, what):
    for k in a:
        x, y = a[k], b[k]
        assert x.dtype == y.dtype and x.shape == y.shape
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (what, k, np.flatnonzero(x.view(np.uint8) != y.view(np.uint8))[:8])


def _pair(m, s, g, what, **kw):
    """the call with one tensor as cost and obstacle map against the call with a cloned obstacle map: the same bits everywhere"""
    stored = _launch(m, s, g, alias=True, **kw)
    general = _launch(m, s, g, alias=False, **kw)
    _same_bits(stored, general, what)
    return stored


def _levels(B, seed):
    return np.random.default_rng(seed).integers(0, 40, B).astype(np.int32)


# ---- 1. every shape, both entry points ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("W", SIZES)
def test_plain_and_ranked_launch_equal_the_general_stream(W, B):
    n = len(_bank(W))
    firsts = range(0, n, B) if B < n else (0, 7)  # the small batches walk through the whole bank
    for first in firsts:
        m, s, g, names = _batch(W, B, first)
        ex = _pair(m, s, g, (W, B, first, "ex"))
        lv = _pair(m, s, g, (W, B, first, "levels"), which="levels", levels=_levels(B, first))
        _same_bits(ex, lv, (W, B, first, "ex vs levels"))
        assert ex["summary"][0] == 1  # the completion flag came up


# ---- 2. against the CPU oracle -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", SIZES)
def test_binary_maps_equal_the_oracle(W):
    from oracle import oracle as O
    B = len(_bank(W))
    m, s, g, names = _batch(W, B)
    keep = _binary(names)
    got = _launch(m, s, g, alias=True, log=True)
    o = O.forward(m[keep], s[keep], g[keep], m[keep], 0.5, W * W, mode="sm", want_log=True)
    hist = got["histories"].reshape(B, W, W)[keep]
    paths = got["paths"].reshape(B, W, W)[keep]
    it = got["iters"][keep]
    assert np.array_equal(it, o.iters)
    assert np.array_equal(hist, o.histories) and np.array_equal(paths, o.paths)
    assert np.array_equal(got["status"][keep] != 0, o.map_status != 0)
    log = got["sel_log"].reshape(B, W * W)[keep]
    for b in range(int(keep.sum())):
        assert np.array_equal(log[b, :it[b]], o.sel_log[b, :it[b]]), b


# ---- 3. step budgets -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", SIZES)
@pytest.mark.parametrize("budget", ["1", "3", "HW-1"])
def test_step_budgets(W, budget):
    max_iters = {"1": 1, "3": 3, "HW-1": W * W - 1}[budget]
    m, s, g, names = _batch(W, 65)
    out = _pair(m, s, g, (W, budget), max_iters=max_iters, log=True)
    assert (out["iters"] <= max_iters).all()
    _pair(m, s, g, (W, budget, "levels"), which="levels", levels=_levels(65, 5), max_iters=max_iters)
    _pair(m, s, g, (W, budget, "routes"), max_iters=max_iters, routes=True)


# ---- 4. g_ratio, the selection log, the coupled marks ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", SIZES)
@pytest.mark.parametrize("g_ratio", [0.5, 0.3, 0.8, 1.0])
@pytest.mark.parametrize("log", [False, True])
def test_g_ratio_with_and_without_log(W, g_ratio, log):
    m, s, g, names = _batch(W, 65, first=3)
    _pair(m, s, g, (W, g_ratio, log), g_ratio=g_ratio, log=log)
    _pair(m, s, g, (W, g_ratio, log, "marks"), g_ratio=g_ratio, log=log, marks=True)
    if not log:
        _pair(m, s, g, (W, g_ratio, "levels"), which="levels", levels=_levels(65, 11), g_ratio=g_ratio)


# ---- 5. routes -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", SIZES)
@pytest.mark.parametrize("g_ratio", [0.5, 0.3])
def test_routes_lengths_and_costs(W, g_ratio):
    B = len(_bank(W))
    m, s, g, names = _batch(W, B)
    out = _pair(m, s, g, (W, g_ratio, "routes"), g_ratio=g_ratio, routes=True, marks=True)
    # a route's cost is the number of its cells that are passable and not the goal: the start counts 0 when it sits on an obstacle
    keep = _binary(names)
    paths = out["paths"].reshape(B, -1)
    for b in np.flatnonzero(keep & (out["status"] == 0)):
        on = paths[b] != 0
        want = float(m[b].reshape(-1)[on].sum() - m[b].reshape(-1)[g[b].reshape(-1) != 0].sum())
        assert out["route_len"][b] == on.sum() and out["route_cost"][b] == want, (names[b], out["route_cost"][b], want)


# ---- 6. the module ---------------------------------------------------------------------------------------------------------------------------
def test_vanilla_astar_forward_equals_the_general_stream():
    from neural_astar.planner import VanillaAstar
    from neural_astar.utils import synthetic as syn
    W, B = 32, 130
    parts = (syn.maze_maps(B // 2, W, seed=77), syn.random_obstacle_maps(B - B // 2, W, W, 0.25, seed=78))
    m, s, g = (np.concatenate([p[k] for p in parts]) for k in range(3))
    va = VanillaAstar().to(_dev()).eval()
    with torch.no_grad():
        out = va(_t(m), _t(s), _t(g))
    torch.cuda.synchronize()
    general = _launch(m[:, 0], s[:, 0], g[:, 0], alias=False)
    assert (general["status"] == 0).all()
    assert np.array_equal(out.histories[:, 0].cpu().numpy().reshape(-1), general["histories"])
    assert np.array_equal(out.paths[:, 0].cpu().numpy().reshape(-1), general["paths"])
