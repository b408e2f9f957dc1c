"""CPU: sampled routes from the tiled soft field's checkpointed tape (include/nastar_soft_routes_tiled.h, ``ops.soft_routes_tiled``) --
everything that needs no GPU.

1. the nineteenth header against ``_native.SOFT_ROUTES_TILED_SIGNATURES``; the library exports the symbols; every refusal the entry point
   makes before any HIP call, and their order; ``workspace_bytes`` at 0 and SIZE_MAX;
2. the Python refusals made before a launch, and the planner methods;
3. the float32 stand-in on the above-limit cases of the GPU tests: no mismatch outside the fragile band, the fragile share within
   ``RO.FRAGILE_MAX_SHARE``, and the log-probability gap ``RC.LOGP_STANDIN`` is measured as; the visits' seed on the float64 oracle.
"""
import inspect

import numpy as np
import pytest
import torch

import soft_fields_oracle as SO
import soft_fields_tiled_cases as TC
import soft_routes_oracle as RO
import soft_routes_tiled_cases as RC
from test_fields import _defines, _prototypes

f32, f64 = np.float32, np.float64
SIZE_MAX = 2 ** 64 - 1
NAMES = ["nastar_soft_routes_tiled", "nastar_soft_routes_tiled_abi", "nastar_soft_routes_tiled_max_cells", "nastar_soft_routes_tiled_workspace_bytes"]
ARGS = ["cost", "goal", "passable", "tape", "tape_bytes", "checkpoint_every", "start_idx", "B", "S", "N", "H", "W", "neighbor_mask", "tau", "horizon",
        "seed", "uniforms", "routes_out", "route_cap", "route_len_out", "route_cost_out", "log_prob_out", "visits_out", "status_out", "workspace",
        "workspace_bytes", "stream"]


# ---- 1: header, binding, library, refusals ----------------------------------------------------------------------------------------------------
def test_nineteenth_header_and_its_signature_table_agree():
    from neural_astar import _native
    protos = _prototypes("nastar_soft_routes_tiled.h")
    assert sorted(protos) == sorted(_native.SOFT_ROUTES_TILED_SIGNATURES) == NAMES
    for name, (ret, args) in protos.items():
        assert _native.SOFT_ROUTES_TILED_SIGNATURES[name] == ret + " " + "".join(k for k, _ in args), name
    assert [n for _, n in protos["nastar_soft_routes_tiled"][1]] == ARGS
    assert [n for _, n in protos["nastar_soft_routes_tiled_workspace_bytes"][1]] == ["B", "S", "N", "H", "W", "horizon", "checkpoint_every"]
    # the call is nastar_soft_routes' with checkpoint_every behind the tape and a workspace in front of the stream
    old = [n for _, n in _prototypes("nastar_soft_routes.h")["nastar_soft_routes"][1]]
    assert [a for a in ARGS if a not in ("checkpoint_every", "workspace", "workspace_bytes")] == old
    # a table of its own: the other tables and headers are what they were
    for table in (_native.SIGNATURES, _native.SOFT_ROUTE_SIGNATURES, _native.SOFT_FIELD_SIGNATURES, _native.SOFT_FIELD_TILED_SIGNATURES,
                  _native.SOFT_POLICY_SIGNATURES, _native.SOFT_POLICY_TILED_SIGNATURES):
        assert not set(_native.SOFT_ROUTES_TILED_SIGNATURES) & set(table)
    assert len(_native.SIGNATURES) == 74 and len(_native.SOFT_ROUTE_SIGNATURES) == 4 == len(_prototypes("nastar_soft_routes.h"))
    assert _defines("nastar_soft_routes_tiled.h") == {"NASTAR_SOFT_ROUTES_TILED_ABI": 1} and _defines("nastar.h")["NASTAR_VERSION"] == 800


def test_library_exports_the_tiled_soft_route_symbols():
    from neural_astar import _native, ops
    lib = _native.load()
    for sym in _native.SOFT_ROUTES_TILED_SIGNATURES:
        assert hasattr(lib, sym), sym
    assert lib.nastar_soft_routes_tiled_abi() == 1
    assert lib.nastar_soft_routes_tiled_max_cells() == lib.nastar_soft_fields_tiled_max_cells() == 1179648 == ops.SOFT_FIELDS_TILED_MAX_CELLS
    assert len(lib.nastar_soft_routes_tiled.argtypes) == 27
    assert {"soft_routes_tiled", "soft_routes_tiled_from_tape"} <= set(ops.__all__)


def test_workspace_bytes_at_zero_at_size_max_and_in_between():
    from neural_astar import _native
    lib = _native.load()
    size = lib.nastar_soft_routes_tiled_workspace_bytes
    good = dict(B=2, S=3, N=5, H=48, W=130, horizon=60, checkpoint_every=8)
    for name in good:
        for bad in (0, -1):
            assert size(*dict(good, **{name: bad}).values()) == 0, name
    assert size(1 << 20, 1 << 15, 1 << 15, 1 << 30, 1 << 30, 1 << 30, 1 << 30) == SIZE_MAX
    assert size(1 << 30, 1 << 30, 1 << 30, 1, 1, 1, 1) == SIZE_MAX                      # the walkers' state alone
    # the flags twice, the costs and V_0, 32 bytes per walker, min(c, K) - 1 planes of the segment
    plane = 2 * 48 * 130 * 4
    assert size(*good.values()) == 2 * 256 + 2 * plane + 2 * 3 * 5 * 32 + 7 * plane
    assert size(*dict(good, checkpoint_every=1).values()) == 2 * 256 + 2 * plane + 2 * 3 * 5 * 32
    assert size(*dict(good, checkpoint_every=500).values()) == 2 * 256 + 2 * plane + 2 * 3 * 5 * 32 + 59 * plane
    assert size(*dict(good, N=6).values()) - size(*good.values()) == 2 * 3 * 32


P = 0x10000  # never dereferenced: every call below is refused on its arguments
TAPE = 2 * 64 * 4 * (16 // 4 + 1)


def _call(**over):
    a = dict(cost=P, goal=P, passable=P, tape=P, tape_bytes=TAPE, checkpoint_every=4, start_idx=P, B=2, S=3, N=5, H=8, W=8, neighbor_mask=0x1EF,
             tau=0.5, horizon=16, seed=7, uniforms=None, routes_out=P, route_cap=17, route_len_out=P, route_cost_out=P, log_prob_out=P,
             visits_out=P, status_out=P, workspace=P, workspace_bytes=1 << 20, stream=None)
    a.update(over)
    return a


@pytest.mark.parametrize("over,rc", [
    (dict(neighbor_mask=0x1FF), 2), (dict(neighbor_mask=0x200), 2), (dict(cost=None), 5), (dict(goal=None), 5), (dict(passable=None), 5),
    (dict(tape=None), 5), (dict(start_idx=None), 5), (dict(route_len_out=None), 5), (dict(status_out=None), 5), (dict(workspace=None), 5),
    (dict(B=0), 1), (dict(S=0), 1), (dict(N=-1), 1), (dict(H=0), 1), (dict(W=-1), 1), (dict(horizon=0), 1), (dict(checkpoint_every=0), 1),
    (dict(checkpoint_every=-3), 1), (dict(tau=0.0), 1), (dict(tau=float("nan")), 1), (dict(tau=float("inf")), 1), (dict(route_cap=0), 1),
    (dict(route_cap=-4), 1),
    (dict(neighbor_mask=0x010, cost=None), 2),           # the mask is looked at first
    (dict(cost=None, B=0), 5),                            # a NULL before the shape
    (dict(N=0, H=1024, W=1153), 1),                       # the shape before the limit
    (dict(H=1024, W=1153), 2), (dict(H=1, W=1179649), 2), (dict(H=65536, W=65536), 2),
    (dict(B=1 << 25, H=1, W=1), 2),                       # more than 2^24 tiles in the batch
    (dict(B=1 << 10, S=1 << 10, N=(1 << 10) + 1), 2),    # more than 2^30 walkers
    (dict(S=1 << 30, N=1 << 30), 2),
    (dict(H=1024, W=1153, tape_bytes=0), 2),              # the limit before the tape
    (dict(tape_bytes=TAPE - 1), 6), (dict(tape=P + 8), 6), (dict(checkpoint_every=3), 6), (dict(horizon=20), 6), (dict(B=3), 6),
    (dict(workspace_bytes=0), 6), (dict(workspace=P + 4), 6), (dict(workspace_bytes=2 * 256 + 2 * 512 + 960 + 3 * 512 - 1), 6)])
def test_soft_routes_tiled_refuses_bad_arguments_without_a_device(over, rc):
    from neural_astar import _native
    lib = _native.load()
    for optional in (dict(), dict(route_cost_out=None, log_prob_out=None, visits_out=None), dict(uniforms=P)):   # any of them may be NULL
        assert lib.nastar_soft_routes_tiled(*_call(**dict(optional, **over)).values()) == rc
    assert lib.nastar_last_error() == b""


def test_route_cap_is_not_looked_at_without_rows():
    from neural_astar import _native
    lib = _native.load()
    assert lib.nastar_soft_routes_tiled(*_call(routes_out=None, route_cap=0, tape_bytes=0).values()) == 6   # (past the shape checks: only the tape is wrong)
    assert lib.nastar_soft_routes_tiled_workspace_bytes(2, 3, 5, 8, 8, 16, 4) == 2 * 256 + 2 * 512 + 960 + 3 * 512


# ---- 2: the Python side ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_before_a_launch_and_the_planner_methods():
    from neural_astar import ops, planner
    from neural_astar.planner.differentiable_astar import DifferentiableAstar
    m = torch.ones(2, 1, 8, 8)
    st = torch.zeros(2, 3, dtype=torch.int64)
    tape = torch.zeros(16, dtype=torch.uint8)
    for call in (lambda **kw: ops.soft_routes_tiled(m, m, m, st, kw.pop("tau", 0.5), **kw),
                 lambda **kw: ops.soft_routes_tiled_from_tape(m, m, m, tape, st, kw.pop("tau", 0.5), **kw)):
        for bad in (0, -1, True, 2.0, None):
            with pytest.raises(ValueError, match="num_samples"):
                call(num_samples=bad)
        for bad in (0, True, 1.5):
            with pytest.raises(ValueError, match="max_route_len"):
                call(max_route_len=bad)
        for bad in (1.5, True, 2 ** 63, "7"):
            with pytest.raises(ValueError, match="seed"):
                call(seed=bad)
        for bad in (0.0, -1.0, float("nan"), float("inf"), True, None):
            with pytest.raises(ValueError, match="tau"):
                call(tau=bad, seed=1)
        for bad in (0, -2, True, 1.5):
            with pytest.raises(ValueError, match="checkpoint_every"):
                call(seed=1, checkpoint_every=bad)
        with pytest.raises(ValueError, match="horizon"):
            call(horizon=0, seed=1)
        with pytest.raises(ValueError, match="neighbor_mask"):
            call(seed=1, neighbor_mask=0x1FF)
    with pytest.raises(TypeError, match="float32"):
        ops.soft_routes_tiled(m.double(), m, m, st, 0.5, seed=1)
    with pytest.raises(ValueError, match="starts"):
        ops.soft_routes_tiled(m, m, m, torch.zeros(3, 3, dtype=torch.int64), 0.5, seed=1)
    wide = torch.ones(1, 1, 1024, 1153)
    for call in (lambda: ops.soft_routes_tiled(wide, wide, wide, torch.zeros(1, 1, dtype=torch.int64), 0.5, seed=1),
                 lambda: ops.soft_routes_tiled_from_tape(wide, wide, wide, tape, torch.zeros(1, 1, dtype=torch.int64), 0.5)):
        with pytest.raises(NotImplementedError, match="1179648"):
            call()
    with pytest.raises(NotImplementedError, match="walkers"):
        ops.soft_routes_tiled_from_tape(m, m, m, tape, st, 0.5, num_samples=1 << 28)
    with pytest.raises(ValueError, match="uniforms"):
        ops.soft_routes_tiled_from_tape(m, m, m, tape, st, 0.5, num_samples=2, uniforms=torch.zeros(2, 3, 2, 31))
    # the one-workgroup call still stops at its limit, and now says where to go
    big = torch.ones(1, 1, 97, 128)
    for call in (lambda: ops.soft_routes(big, big, big, torch.zeros(1, 1, dtype=torch.int64), 0.5, seed=1),
                 lambda: ops.soft_routes_from_tape(big, big, big, tape, torch.zeros(1, 1, dtype=torch.int64), 0.5)):
        with pytest.raises(NotImplementedError, match="12288.*soft_routes_tiled"):
            call()
    # the signatures: ops, and the planners' tiled method beside sample_routes, whose own signature is what it was
    assert str(inspect.signature(ops.soft_routes_tiled)) == str(inspect.signature(ops.soft_routes)).replace(
        ") -> 'SoftRoutes'", ", checkpoint_every: 'Optional[int]' = None) -> 'SoftRoutes'")
    assert str(inspect.signature(ops.soft_routes_tiled_from_tape)) == str(inspect.signature(ops.soft_routes_from_tape)).replace(
        "shape: 'Optional[str]'", "checkpoint_every: 'Optional[int]'")
    for cls in (DifferentiableAstar, planner.VanillaAstar, planner.NeuralAstar):
        old, new = str(inspect.signature(cls.sample_routes)), str(inspect.signature(cls.sample_routes_tiled))
        assert new == old.replace("visits: 'bool' = False)", "visits: 'bool' = False, checkpoint_every: 'Optional[int]' = None)"), cls
        assert "tiled" not in old
    with pytest.raises(NotImplementedError, match="encoder_input"):
        planner.NeuralAstar(encoder_input="m+").sample_routes_tiled(m, st, m, 0.5)
    na = planner.NeuralAstar(encoder_input="m")
    with pytest.raises(ValueError, match="max_route_len"):
        na.sample_routes_tiled(m, st, m, 0.5, max_route_len=0)
    with pytest.raises(ValueError, match="tau"):
        na.sample_routes_tiled(m, st, m, 0.0)
    with pytest.raises(ValueError, match="num_samples"):
        na.sample_routes_tiled(m, st, m, 0.5, num_samples=0)


# ---- 3: the float32 stand-in on the GPU tests' cases ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,B,seed,K", RC.ABOVE, ids=lambda v: str(v))
def test_float32_stand_in_draws_the_oracles_routes_outside_the_fragile_band(H, W, B, seed, K):
    cost, passable, goal = TC.maps(H, W, B, seed)
    worst_share, worst_gap = 0.0, 0.0
    for mask in RC.ABOVE_MASKS:
        for tau in RC.ABOVE_TAUS:
            what = f"{H}x{W} K={K} tau={tau} mask={mask:#05x}"
            starts = RC.above_starts(H, W, B, seed, K, mask)
            total = flagged = 0
            gap = 0.0
            for b in range(B):
                planes32 = SO.soft_field(cost[b], goal[b], passable[b], tau, K, mask, f32).planes
                groups = RC.above_groups(b, starts, B)
                ref = RO.walk_many(planes32, cost[b], goal[b], passable[b], groups, tau, mask)[0]
                got = RO.walk_many(planes32, cost[b], goal[b], passable[b], groups, tau, mask, dtype=f32)[0]
                assert np.array_equal(ref.status, got.status), what
                live = ref.status == 0
                total, flagged = total + int(live.sum()), flagged + int(ref.fragile[live].sum())
                assert all(ref.cells[k] == got.cells[k] for k in np.flatnonzero(live & ~ref.fragile)), what      # 0 mismatches
                n0 = groups[0][0]
                d0 = np.where(goal[b].reshape(-1)[n0[live]] != 0, 0.0, np.asarray(planes32[K], f64).reshape(-1)[n0[live]])
                gap = max(gap, float(np.abs(got.log_prob[live] - (d0 - got.cost[live]) / tau).max() / RO.logp_scale(planes32, tau)))
            share = flagged / total
            print(f"{what}: {total} routes, {flagged} fragile ({share:.4f}), log-prob gap {gap:.3e}")
            assert total >= 3 * RC.ABOVE_N * B and share <= RO.FRAGILE_MAX_SHARE, what      # (the two near starts and the goal walk)
            worst_share, worst_gap = max(worst_share, share), max(worst_gap, gap)
    assert worst_share <= RC.STANDIN_FRAGILE                                           # (the figures the cases file quotes as measured)
    if (H, W) == RC.ABOVE[1][:2]:
        assert worst_gap <= RC.LOGP_STANDIN and RC.LOGP_RTOL == 4 * max(RC.LOGP_STANDIN, RC.LOGP_KERNELS)


def test_the_visits_seed_on_the_float64_oracle():
    """the seed of the GPU test's 4096 routes, on the oracle's own visits first: inside the bound with room to spare"""
    cost, passable, goal, start = TC.maxent_maps()
    H, W, K = cost.shape[1], cost.shape[2], TC.ABOVE[1][4]
    tau, N = RC.VISITS_TAU, RC.VISITS_N
    n0 = int(np.flatnonzero(start[0].reshape(-1))[0])
    assert SO.hops(goal[0], passable[0]).reshape(-1)[n0] == 40
    fld = SO.soft_field(cost[0], goal[0], passable[0], tau, K, SO.MOORE8, f64)
    expect = SO.soft_field_grad(cost[0], goal[0], passable[0], start[0].astype(f64), tau, K).grad.reshape(-1)
    r = RO.walk(fld.planes, cost[0], goal[0], passable[0], np.full(N, n0), tau, SO.MOORE8, lambda j: RO.uniform(RC.VISITS_SEED, 0, np.arange(N), j))
    per = np.zeros((N, H * W), f32)
    for i, cells in enumerate(r.cells):
        np.add.at(per[i], cells[:-1], 1)
    ratio = np.abs(per.astype(f64).mean(0) - expect) / RC.visits_bound(per, expect, N, SO.BWD_RTOL * np.abs(expect).max())
    print(f"visits / N of the oracle against the adjoint: worst cell at {ratio.max():.3f} of its bound")
    assert (r.status == 0).all() and ratio.max() <= 0.75
