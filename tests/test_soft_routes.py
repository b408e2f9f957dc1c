"""CPU: sampled routes from the maximum-entropy route distribution (include/nastar_soft_routes.h, ``ops.soft_routes``) -- everything that
needs no GPU.

1. Philox4x32-10 of tests/soft_routes_oracle.py against its known answers;
2. the eighteenth header against ``_native.SOFT_ROUTE_SIGNATURES``; the library exports the symbols; every refusal the entry point makes
   before any HIP call, and their order;
3. the numpy definition on maps one can check by hand: a corridor has one route whatever u; u = 0 takes the first candidate, u just below
   1 the last; a start on a goal, an obstacle, outside the map; the identity log p = (V_K(n_0) - cost) / tau in float64; the empirical
   visits against the adjoint of tests/soft_fields_oracle.py;
4. the float32 stand-in on the cases of the GPU tests: the share of fragile routes, no mismatch among the others, and the log-probability
   gap ``RO.LOGP_STANDIN`` is measured as;
5. the Python refusals made before a launch, and the planner methods.
"""
import inspect

import numpy as np
import pytest
import torch

import heuristic_oracle as HO
import soft_fields_oracle as SO
import soft_routes_oracle as RO
from test_fields import _defines, _prototypes

f32, f64 = np.float32, np.float64
NAMES = ["nastar_soft_routes", "nastar_soft_routes_abi", "nastar_soft_routes_max_cells", "nastar_soft_routes_with_shape"]
ARGS = ["cost", "goal", "passable", "tape", "tape_bytes", "start_idx", "B", "S", "N", "H", "W", "neighbor_mask", "tau", "horizon", "seed",
        "uniforms", "routes_out", "route_cap", "route_len_out", "route_cost_out", "log_prob_out", "visits_out", "status_out"]


# ---- 1: the generator ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counter,key,out", RO.PHILOX_KNOWN)
def test_philox_known_answers(counter, key, out):
    assert [int(x) for x in RO.philox4x32_10(counter, key)] == list(out)


def test_philox_broadcasts_and_the_uniform_is_24_bits():
    j = np.arange(7)
    u = RO.uniform(-3, 5, 2, j)  # (a negative seed is its 64-bit pattern)
    assert u.shape == (7,) and ((0 <= u) & (u < 1)).all() and np.array_equal(u * 2 ** 24, np.floor(u * 2 ** 24))
    for k in range(7):
        x0 = RO.philox4x32_10((k, 2, 5, 0), (0xfffffffd, 0xffffffff))[0]
        assert u[k] == (int(x0) >> 8) / 2 ** 24
    assert len(set(u.tolist())) == 7 and not np.array_equal(u, RO.uniform(-3, 5, 3, j)) and not np.array_equal(u, RO.uniform(-3, 6, 2, j))


# ---- 2: header, binding, library, refusals ----------------------------------------------------------------------------------------------------
def test_eighteenth_header_and_soft_route_signatures_agree():
    from neural_astar import _native
    protos = _prototypes("nastar_soft_routes.h")
    assert sorted(protos) == sorted(_native.SOFT_ROUTE_SIGNATURES) == NAMES
    for name, (ret, args) in protos.items():
        assert _native.SOFT_ROUTE_SIGNATURES[name] == ret + " " + "".join(k for k, _ in args), name
    assert [n for _, n in protos["nastar_soft_routes"][1]] == ARGS + ["stream"]
    assert [n for _, n in protos["nastar_soft_routes_with_shape"][1]] == ARGS + ["shape", "stream"]
    # a table of its own: the other tables and headers are what they were
    for table in (_native.SIGNATURES, _native.FIELD_ROUTE_SIGNATURES, _native.SOFT_FIELD_SIGNATURES, _native.SOFT_FIELD_TILED_SIGNATURES,
                  _native.SOFT_POLICY_SIGNATURES, _native.SOFT_POLICY_TILED_SIGNATURES):
        assert not set(_native.SOFT_ROUTE_SIGNATURES) & set(table)
    assert len(_native.SIGNATURES) == 74 and len(_native.SOFT_FIELD_SIGNATURES) == 6 == len(_prototypes("nastar_soft_fields.h"))
    assert _defines("nastar_soft_routes.h") == {"NASTAR_SOFT_ROUTES_ABI": 1} and _defines("nastar.h")["NASTAR_VERSION"] == 800


def test_library_exports_the_soft_route_symbols():
    from neural_astar import _native, ops
    lib = _native.load()
    for sym in _native.SOFT_ROUTE_SIGNATURES:
        assert hasattr(lib, sym), sym
    assert lib.nastar_soft_routes_abi() == 1
    assert lib.nastar_soft_routes_max_cells() == lib.nastar_soft_fields_max_cells() == 12288 == ops.SOFT_ROUTES_MAX_CELLS
    assert len(lib.nastar_soft_routes.argtypes) == 24 and len(lib.nastar_soft_routes_with_shape.argtypes) == 25
    assert {"soft_routes", "SoftRoutes", "soft_routes_from_tape", "SOFT_ROUTES_MAX_CELLS"} <= set(ops.__all__)
    assert ops.SoftRoutes._fields == ("routes", "route_lengths", "route_costs", "log_probs", "visits", "dists", "status", "map_status")


P = 0x10000  # never dereferenced: every call below is refused on its arguments


def _call(**over):
    a = dict(cost=P, goal=P, passable=P, tape=P, tape_bytes=2 * 64 * 16 * 4, start_idx=P, B=2, S=3, N=5, H=8, W=8, neighbor_mask=0x1EF, tau=0.5,
             horizon=16, seed=7, uniforms=None, routes_out=P, route_cap=17, route_len_out=P, route_cost_out=P, log_prob_out=P, visits_out=P,
             status_out=P, stream=None)
    a.update(over)
    return a


@pytest.mark.parametrize("over,rc", [
    (dict(neighbor_mask=0x1FF), 2), (dict(neighbor_mask=0x200), 2), (dict(cost=None), 5), (dict(goal=None), 5), (dict(passable=None), 5),
    (dict(tape=None), 5), (dict(start_idx=None), 5), (dict(route_len_out=None), 5), (dict(status_out=None), 5),
    (dict(B=0), 1), (dict(S=0), 1), (dict(N=-1), 1), (dict(H=0), 1), (dict(W=-1), 1), (dict(horizon=0), 1), (dict(tau=0.0), 1),
    (dict(tau=float("nan")), 1), (dict(tau=float("inf")), 1), (dict(route_cap=0), 1), (dict(route_cap=-4), 1),
    (dict(neighbor_mask=0x010, cost=None), 2),           # the mask is looked at first
    (dict(cost=None, B=0), 5),                            # a NULL before the shape
    (dict(N=0, H=128, W=129), 1),                         # the shape before the limit
    (dict(H=97, W=128), 2), (dict(H=1, W=12289), 2), (dict(H=65536, W=65536), 2),
    (dict(B=1 << 10, S=1 << 10, N=(1 << 10) + 1), 2),    # more than 2^30 walkers
    (dict(S=1 << 30, N=1 << 30), 2),
    (dict(H=97, W=128, tape_bytes=0), 2),                 # the limit before the tape
    (dict(tape_bytes=2 * 64 * 16 * 4 - 1), 6), (dict(tape=P + 8), 6), (dict(horizon=17), 6), (dict(B=3), 6)])
def test_soft_routes_refuses_bad_arguments_without_a_device(over, rc):
    from neural_astar import _native
    lib = _native.load()
    for optional in (dict(), dict(route_cost_out=None, log_prob_out=None, visits_out=None), dict(uniforms=P)):   # any of them may be NULL
        a = _call(**dict(optional, **over))
        assert lib.nastar_soft_routes(*a.values()) == rc
        head, stream = list(a.values())[:-1], a["stream"]
        for shape in (0, 1, 2):
            assert lib.nastar_soft_routes_with_shape(*head, shape, stream) == rc
    assert lib.nastar_last_error() == b""


def test_route_cap_is_not_looked_at_without_rows_and_a_shape_outside_its_range_is_refused():
    from neural_astar import _native
    lib = _native.load()
    a = _call(routes_out=None, route_cap=0, tape_bytes=0)
    assert lib.nastar_soft_routes(*a.values()) == 6       # (past the shape checks: only the tape is wrong)
    head = list(_call().values())[:-1]
    assert lib.nastar_soft_routes_with_shape(*head, 3, None) == 1 and lib.nastar_soft_routes_with_shape(*head, -1, None) == 1


# ---- 3: the definition, by hand ------------------------------------------------------------------------------------------------------------------
def _field(cost, goal, passable, tau, K, mask=HO.MOORE8, dtype=f64):
    return SO.soft_field(np.asarray(cost, f32), np.asarray(goal, f32), np.asarray(passable, f32), tau, K, mask, dtype)


@pytest.mark.parametrize("u", [0.0, 0.3, 1.0 - 2.0 ** -24, 1.0, float("nan")])
def test_a_corridor_has_one_route_whatever_u(u):
    W = 9
    cost = np.linspace(0.25, 1.0, W, dtype=f32)[None]
    goal = np.zeros((1, W), f32)
    goal[0, W - 1] = 1
    ok = np.ones((1, W), f32)
    fld = _field(cost, goal, ok, 0.5, W + 3, SO.DIRECTED)  # right and down only: one candidate per move
    r = RO.walk(fld.planes, cost, goal, ok, [0, 3, W - 1], 0.5, SO.DIRECTED, lambda j: np.full(3, u))
    assert r.cells == [list(range(W)), list(range(3, W)), [W - 1]] and r.status.tolist() == [0, 0, 0] and not r.fragile.any()
    assert np.allclose(r.cost, [cost[0, :-1].sum(), cost[0, 3:-1].sum(), 0]) and np.allclose(r.log_prob, 0, atol=1e-12)
    # two-way moves: the walker may turn back, and a horizon of exactly the distance leaves one route again
    exact = _field(cost, goal, ok, 0.5, W - 1, 0x028)       # left and right
    r = RO.walk(exact.planes, cost, goal, ok, [0], 0.5, 0x028, lambda j: np.full(1, u))
    assert r.cells == [list(range(W))] and abs(r.log_prob[0]) < 1e-12


def test_u_zero_takes_the_first_candidate_and_u_below_one_the_last():
    H = W = 5
    cost = np.full((H, W), 0.5, f32)
    goal = np.zeros((H, W), f32)
    goal[0, :] = goal[-1, :] = goal[:, 0] = goal[:, -1] = 1   # a ring of goals: every move from the centre ends the route
    ok = np.ones((H, W), f32)
    centre = 2 * W + 2
    for mask, moves in ((HO.MOORE8, SO.ACTION_MOVES), (HO.VON_NEUMANN, SO.ACTION_MOVES[:4])):
        fld = _field(cost, goal, ok, 1.0, 4, mask)
        # plane K-1 = V_3 around (2,2): the eight neighbours are no goals; from (1,1) etc. the route goes on
        first = RO.walk(fld.planes, cost, goal, ok, [centre], 1.0, mask, lambda j: np.zeros(1))
        last = RO.walk(fld.planes, cost, goal, ok, [centre], 1.0, mask, lambda j: np.full(1, 1.0 - 2.0 ** -24))
        dy, dx = moves[0]
        assert first.cells[0][1] == centre + dy * W + dx and first.cells[0][2] == centre + 2 * (dy * W + dx)
        dy, dx = moves[-1]
        assert last.cells[0][1] == centre + dy * W + dx
        assert first.cells[0][-1] != centre and goal.reshape(-1)[first.cells[0][-1]] and goal.reshape(-1)[last.cells[0][-1]]
        over = RO.walk(fld.planes, cost, goal, ok, [centre], 1.0, mask, lambda j: np.full(1, 7.0))
        assert over.cells == last.cells


def test_failed_queries_and_a_start_on_a_goal():
    cost = np.full((3, 4), 0.5, f32)
    ok = np.ones((3, 4), f32)
    ok[:, 2] = 0                       # a wall: column 3 is cut off
    goal = np.zeros((3, 4), f32)
    goal[0, 0] = goal[1, 2] = 1        # a passable goal and a goal on the wall
    fld = _field(cost, goal, ok, 0.5, 8)
    r = RO.walk(fld.planes, cost, goal, ok, [0, 6, 7, 2, -1, 12, 5], 0.5, HO.MOORE8, lambda j: np.full(7, 0.5))
    assert r.status.tolist() == [0, 0, 3, 3, 1, 1, 0]
    assert r.cells[0] == [0] and r.cells[1] == [6] and r.cells[2] == r.cells[3] == r.cells[4] == r.cells[5] == []
    assert r.cost[:2].tolist() == [0, 0] and r.log_prob[:2].tolist() == [0, 0] and np.isposinf(r.cost[2:6]).all() and np.isneginf(r.log_prob[2:6]).all()
    assert r.cells[6][0] == 5 and r.cells[6][-1] == 0 and 6 not in r.cells[6] and 2 not in r.cells[6]   # the goal on the wall is never entered
    bad = RO.walk(None, cost, goal, ok, [0, -1], 0.5, HO.MOORE8, lambda j: np.zeros(2))
    assert bad.status.tolist() == [9, 1] and bad.cells == [[], []]
    assert np.array_equal(RO.padded([[1, 2, 3, 4], [9], []], 3), [[2, 3, 4], [9, -1, -1], [-1, -1, -1]])
    assert RO.visits([[1, 2, 1, 4], [4], []], 6).tolist() == [0, 2, 1, 0, 0, 0]


@pytest.mark.parametrize("tau", [1.0, 0.1, 0.02])
@pytest.mark.parametrize("mask", SO.MASKS)
def test_log_prob_is_the_field_at_the_start_minus_the_cost_over_tau(tau, mask):
    H, W, N = 9, 11, 64
    cost, passable, goal = SO.random_maps(21, 1, H, W)
    K = SO.default_horizon(H, W)
    fld = _field(cost[0], goal[0], passable[0], tau, K, mask)
    starts = np.repeat(np.flatnonzero(np.isfinite(fld.dist.reshape(-1)))[:6], N)
    r = RO.walk(fld.planes, cost[0], goal[0], passable[0], starts, tau, mask, lambda j: RO.uniform(99, starts, np.arange(starts.size), j))
    assert (r.status == 0).all()
    ref = (fld.dist.reshape(-1)[starts] - r.cost) / tau
    assert np.abs(r.log_prob - ref).max() <= 1e-9 * RO.logp_scale(fld.planes, tau)
    assert len({tuple(c) for c in r.cells}) > (6 if tau == 1.0 and mask != SO.DIRECTED else 0)   # (it does sample)
    for cells in r.cells:   # every route is one the definition allows
        assert goal[0].reshape(-1)[cells[-1]] and not goal[0].reshape(-1)[cells[:-1]].any() and passable[0].reshape(-1)[cells[1:]].all()
        assert len(cells) <= K + 1 and all((((b // W) - (a // W)), ((b % W) - (a % W))) in HO.offsets(mask) for a, b in zip(cells, cells[1:]))


def test_visits_of_the_oracle_are_the_adjoint_of_the_field():
    H = W = 8
    cost, passable, goal = SO.random_maps(3, 1, H, W)
    tau, K, N = 0.5, SO.default_horizon(H, W), 4096
    fld = _field(cost[0], goal[0], passable[0], tau, K)
    n0 = int(np.flatnonzero(np.isfinite(fld.dist.reshape(-1)) & (goal[0].reshape(-1) == 0))[0])
    G = np.zeros((H, W))
    G.reshape(-1)[n0] = 1
    expect = SO.soft_field_grad(cost[0], goal[0], passable[0], G, tau, K).grad.reshape(-1)
    r = RO.walk(fld.planes, cost[0], goal[0], passable[0], np.full(N, n0), tau, HO.MOORE8, lambda j: RO.uniform(5, 0, np.arange(N), j))
    per = np.stack([RO.visits([c], H * W) for c in r.cells]).astype(f64)
    se = per.std(0, ddof=1) / np.sqrt(N)
    # (5 / N: a cell no route or one route stood on has no usable empirical variance; an expectation of 5 / N is missed by all N routes
    # with probability exp(-5))
    assert (np.abs(per.mean(0) - expect) <= 5 * se + 5 / N).all()
    assert per.mean(0)[n0] >= 1 and abs(per.mean(0).sum() - (np.array([len(c) for c in r.cells]) - 1).mean()) < 1e-9


# ---- 4: the float32 stand-in on the GPU tests' cases ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,B,seed", RO.SHAPE_CASES + (RO.BIG_CASE,), ids=lambda v: str(v))
def test_float32_stand_in_draws_the_oracles_routes_outside_the_fragile_band(H, W, B, seed):
    cost, passable, goal = RO.case_maps(H, W, B, seed)
    worst_share, worst_gap = 0.0, 0.0
    for K, tau, mask, walkers in RO.oracle_cases(H, W, B, seed):
        what = f"{H}x{W} K={K} tau={tau} mask={mask:#05x}"
        total = flagged = 0
        for b in range(B):
            planes32 = _field(cost[b], goal[b], passable[b], tau, K, mask, f32).planes
            groups = []                                       # every walker count, Philox and the crafted uniforms: one walk per map
            for (S, N), sample_seed in walkers:
                starts = RO.case_starts(sample_seed, S, passable, goal)
                sel = slice(b * S * N, (b + 1) * S * N)
                philox = RO.case_uniforms(sample_seed, B, S, N)
                uni = RO.crafted_uniforms(sample_seed, B, S, N, K).reshape(-1, K).astype(f64)
                groups.append((np.repeat(starts[b], N), lambda j, u=philox, sel=sel: u(j)[sel]))
                groups.append((np.repeat(starts[b], N), lambda j, u=uni, sel=sel: u[sel, j]))
            refs = RO.walk_many(planes32, cost[b], goal[b], passable[b], groups, tau, mask)
            gots = RO.walk_many(planes32, cost[b], goal[b], passable[b], groups, tau, mask, dtype=f32)
            for (n0, _), ref, got in zip(groups, refs, gots):
                assert np.array_equal(ref.status, got.status), what
                live = ref.status == 0
                if not live.any():
                    continue
                total, flagged = total + int(live.sum()), flagged + int(ref.fragile[live].sum())
                assert all(ref.cells[k] == got.cells[k] for k in np.flatnonzero(live & ~ref.fragile)), what
                d0 = np.where(goal[b].reshape(-1)[n0[live]] != 0, 0.0, np.asarray(planes32[K], f64).reshape(-1)[n0[live]])
                gap = np.abs(got.log_prob[live] - (d0 - got.cost[live]) / tau).max() / RO.logp_scale(planes32, tau)
                worst_gap = max(worst_gap, gap)
        share = flagged / total if total else 0.0
        worst_share = max(worst_share, share)
        assert share <= RO.FRAGILE_MAX_SHARE, (what, total, flagged)
    print(f"{B}x{H}x{W}: worst fragile share {worst_share:.4f}, worst log-prob gap {worst_gap:.3e}")
    assert worst_share <= RO.FRAGILE_MEASURED[0] and worst_gap <= RO.LOGP_STANDIN   # (the figures the oracle file quotes as measured)
    assert RO.LOGP_RTOL == 4 * max(RO.LOGP_STANDIN, RO.LOGP_KERNELS)


# ---- 5: the Python side ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_before_a_launch_and_the_planner_methods():
    from neural_astar import ops, planner
    from neural_astar.planner.differentiable_astar import DifferentiableAstar
    m = torch.ones(2, 1, 8, 8)
    st = torch.zeros(2, 3, dtype=torch.int64)
    tape = torch.zeros(16, dtype=torch.uint8)
    for bad in (0, -1, True, 2.0, None):
        with pytest.raises(ValueError, match="num_samples"):
            ops.soft_routes(m, m, m, st, 0.5, num_samples=bad)
    for bad in (0, True, 1.5):
        with pytest.raises(ValueError, match="max_route_len"):
            ops.soft_routes(m, m, m, st, 0.5, max_route_len=bad)
    for bad in (1.5, True, 2 ** 63, "7"):
        with pytest.raises(ValueError, match="seed"):
            ops.soft_routes(m, m, m, st, 0.5, seed=bad)
    for bad in (0.0, -1.0, float("nan"), float("inf"), True, None):
        with pytest.raises(ValueError, match="tau"):
            ops.soft_routes(m, m, m, st, bad, seed=1)
    with pytest.raises(ValueError, match="horizon"):
        ops.soft_routes(m, m, m, st, 0.5, horizon=0, seed=1)
    with pytest.raises(ValueError, match="neighbor_mask"):
        ops.soft_routes(m, m, m, st, 0.5, seed=1, neighbor_mask=0x1FF)
    with pytest.raises(TypeError, match="float32"):
        ops.soft_routes(m.double(), m, m, st, 0.5, seed=1)
    with pytest.raises(ValueError, match="starts"):
        ops.soft_routes(m, m, m, torch.zeros(3, 3, dtype=torch.int64), 0.5, seed=1)
    with pytest.raises(TypeError, match="starts"):
        ops.soft_routes(m, m, m, st.bool(), 0.5, seed=1)
    big = torch.ones(1, 1, 97, 128)
    with pytest.raises(NotImplementedError, match="12288"):
        ops.soft_routes(big, big, big, torch.zeros(1, 1, dtype=torch.int64), 0.5, seed=1)
    with pytest.raises(NotImplementedError, match="12288"):
        ops.soft_routes_from_tape(big, big, big, tape, torch.zeros(1, 1, dtype=torch.int64), 0.5)
    with pytest.raises(NotImplementedError, match="walkers"):
        ops.soft_routes_from_tape(m, m, m, tape, st, 0.5, num_samples=1 << 28)
    with pytest.raises(ValueError, match="uniforms"):
        ops.soft_routes_from_tape(m, m, m, tape, st, 0.5, num_samples=2, uniforms=torch.zeros(2, 3, 2, 31))
    with pytest.raises(ValueError, match="shape"):
        ops.soft_routes_from_tape(m, m, m, tape, st, 0.5, shape="fast")
    # the existing calls refuse what they refused: a tape above the backward's limit
    mid = torch.ones(1, 1, 64, 97)
    with pytest.raises(NotImplementedError, match="6144"):
        ops.soft_fields_forward(mid, mid, mid, 0.5, tape=True)
    # a seed of None comes from torch's default generator: the same after the same manual_seed
    torch.manual_seed(11)
    a = ops._checked_seed(None)
    torch.manual_seed(11)
    assert a == ops._checked_seed(None) and 0 <= a < 2 ** 63 and ops._checked_seed(-5) == -5
    # the planners: the signatures, and the refusals NeuralAstar makes before its encoder launches anything
    sig = "tau: 'float', num_samples: 'int' = 1, seed: 'Optional[int]' = None, horizon: 'Optional[int]' = None, max_route_len: 'Optional[int]' = None, visits: 'bool' = False)"
    assert str(inspect.signature(DifferentiableAstar.sample_routes)).startswith(
        "(self, cost_maps: 'torch.Tensor', starts: 'torch.Tensor', goal_maps: 'torch.Tensor', obstacles_maps: 'torch.Tensor', " + sig)
    for cls in (planner.VanillaAstar, planner.NeuralAstar):
        assert str(inspect.signature(cls.sample_routes)) == "(self, map_designs: 'torch.Tensor', starts: 'torch.Tensor', goal_maps: 'torch.Tensor', " + sig
    with pytest.raises(NotImplementedError, match="encoder_input"):
        planner.NeuralAstar(encoder_input="m+").sample_routes(m, st, m, 0.5)
    na = planner.NeuralAstar(encoder_input="m")
    with pytest.raises(ValueError, match="max_route_len"):
        na.sample_routes(m, st, m, 0.5, max_route_len=0)
    with pytest.raises(ValueError, match="tau"):
        na.sample_routes(m, st, m, 0.0)
    with pytest.raises(ValueError, match="num_samples"):
        na.sample_routes(m, st, m, 0.5, num_samples=0)
    with pytest.raises(ValueError, match="tau"):
        planner.NeuralAstar(encoder_input="m+").sample_routes(m, st, m, -1.0)   # (the argument checks come before the "m+" refusal, as in plan_many)
