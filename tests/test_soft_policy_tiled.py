"""CPU: the log-policy of the tiled entropy-regularised cost-to-go field and the gradient through it (include/nastar_soft_policy_tiled.h,
``ops.soft_policy_tiled``, ``ops.soft_policy_nll_tiled``) -- everything that needs no GPU.

1. the seventeenth header against ``_native.SOFT_POLICY_TILED_SIGNATURES``; the tables of the other headers are what they were;
2. the library exports the symbols; the workspace function is its sibling's;
3. every refusal the entry points make before any HIP call, and their order; both seeds NULL is not a refusal;
4. the Python refusals made before a launch, and the planner methods; ``soft_policy_nll`` keeps its parameter list;
5. the float32 restatement of the definition on the cases the GPU tests hold to ``PTILED_RTOL``, and the imitation-loss case itself.
"""
import inspect

import numpy as np
import pytest
import torch

import soft_fields_oracle as SO
import soft_fields_tiled_cases as TC
import soft_policy_oracle as PO
import soft_policy_tiled_cases as PC
from test_fields import _defines, _prototypes

f32, f64 = np.float32, np.float64
NAMES = ["nastar_soft_policy_backward_tiled", "nastar_soft_policy_forward_tiled", "nastar_soft_policy_forward_tiled_with_sweeps",
         "nastar_soft_policy_tiled_abi", "nastar_soft_policy_tiled_backward_workspace_bytes"]
FWD_ARGS = ["cost", "goal", "passable", "B", "H", "W", "neighbor_mask", "tau", "horizon", "dist_out", "policy_out", "log_policy_out", "status_out",
            "tape", "tape_bytes", "checkpoint_every", "workspace", "workspace_bytes"]
SIZE_MAX = 2 ** 64 - 1


# ---- 1, 2: header, binding, library ---------------------------------------------------------------------------------------------------------------
def test_seventeenth_header_and_tiled_soft_policy_signatures_agree():
    from neural_astar import _native
    protos = _prototypes("nastar_soft_policy_tiled.h")
    assert sorted(protos) == sorted(_native.SOFT_POLICY_TILED_SIGNATURES) == NAMES
    for name, (ret, args) in protos.items():
        assert _native.SOFT_POLICY_TILED_SIGNATURES[name] == ret + " " + "".join(k for k, _ in args), name
    assert [n for _, n in protos["nastar_soft_policy_forward_tiled"][1]] == FWD_ARGS + ["stream"]
    assert [n for _, n in protos["nastar_soft_policy_forward_tiled_with_sweeps"][1]] == FWD_ARGS + ["sweeps_per_launch", "stream"]
    assert [n for _, n in protos["nastar_soft_policy_backward_tiled"][1]] == [
        "cost", "goal", "passable", "tape", "tape_bytes", "checkpoint_every", "grad_dist", "grad_log_policy", "B", "H", "W", "neighbor_mask", "tau",
        "horizon", "grad_cost_out", "status_out", "workspace", "workspace_bytes", "stream"]
    # the new pointers stand where the one-workgroup policy calls have them: behind policy_out, behind grad_dist
    field_fwd = [n for _, n in _prototypes("nastar_soft_fields_tiled.h")["nastar_soft_cost_to_go_tiled"][1]]
    field_bwd = [n for _, n in _prototypes("nastar_soft_fields_tiled.h")["nastar_soft_fields_backward_tiled"][1]]
    assert [n for n in FWD_ARGS + ["stream"] if n != "log_policy_out"] == field_fwd
    assert [n for _, n in protos["nastar_soft_policy_backward_tiled"][1] if n != "grad_log_policy"] == field_bwd
    # a table of its own: the other tables and headers are what they were
    for table in (_native.SIGNATURES, _native.FIELD_SIGNATURES, _native.TILED_FIELD_SIGNATURES, _native.SOFT_FIELD_SIGNATURES,
                  _native.SOFT_FIELD_TILED_SIGNATURES, _native.SOFT_POLICY_SIGNATURES):
        assert not set(_native.SOFT_POLICY_TILED_SIGNATURES) & set(table)
    assert len(_native.SIGNATURES) == 74 and len(_native.SOFT_FIELD_TILED_SIGNATURES) == 9 and len(_native.SOFT_POLICY_SIGNATURES) == 3
    assert len(_prototypes("nastar_soft_fields_tiled.h")) == 9 and len(_prototypes("nastar_soft_policy.h")) == 3
    assert _defines("nastar_soft_policy_tiled.h") == {"NASTAR_SOFT_POLICY_TILED_ABI": 1}       # no new code, no new version
    assert _defines("nastar_soft_policy.h") == {"NASTAR_SOFT_POLICY_ABI": 1} and _defines("nastar.h")["NASTAR_VERSION"] == 800


def test_library_exports_the_tiled_soft_policy_symbols():
    from neural_astar import _native, ops
    lib = _native.load()
    for sym in _native.SOFT_POLICY_TILED_SIGNATURES:
        assert hasattr(lib, sym), sym
    assert lib.nastar_soft_policy_tiled_abi() == 1
    assert len(lib.nastar_soft_policy_forward_tiled.argtypes) == 19 == len(lib.nastar_soft_policy_backward_tiled.argtypes)
    assert len(lib.nastar_soft_policy_forward_tiled_with_sweeps.argtypes) == 20
    assert {"soft_policy_tiled", "soft_policy_nll_tiled", "soft_policy_tiled_forward", "soft_policy_tiled_backward"} <= set(ops.__all__)


def test_backward_workspace_bytes_are_the_fields():
    from neural_astar import _native
    lib = _native.load()
    size, field = lib.nastar_soft_policy_tiled_backward_workspace_bytes, lib.nastar_soft_fields_tiled_backward_workspace_bytes
    big = 2 ** 31 - 1
    assert [size(0, 4, 4, 4, 2), size(4, 0, 4, 4, 2), size(4, 4, -1, 4, 2), size(4, 4, 4, 0, 2), size(4, 4, 4, 4, 0), size(4, 4, 4, 4, -7)] == [0] * 6
    assert size(big, 1024, 1152, big, big) == SIZE_MAX
    # Q and the live bytes of the injected step stay in LDS: nothing more in device memory
    for B, H, W, K, c in [(1, 1, 1, 1, 1), (2, 32, 33, 130, 12), (3, 67, 69, 97, 1), (1, 1024, 1152, 8, 3), (4, 512, 512, 2048, 46)]:
        assert 0 < size(B, H, W, K, c) == field(B, H, W, K, c), (B, H, W, K, c)


# ---- 3: refusals, made before any HIP call -----------------------------------------------------------------------------------------------------------
P = 0x10000  # never dereferenced: every call below is refused on its arguments
BIG = 1 << 40


def _fwd(**over):
    a = dict(cost=P, goal=P, passable=P, B=2, H=8, W=8, neighbor_mask=0x1EF, tau=0.5, horizon=16, dist_out=P, policy_out=None, log_policy_out=P,
             status_out=P, tape=None, tape_bytes=0, checkpoint_every=4, workspace=P, workspace_bytes=BIG, stream=None)
    a.update(over)
    return a


def _bwd(**over):
    a = dict(cost=P, goal=P, passable=P, tape=P, tape_bytes=2 * 64 * 5 * 4, checkpoint_every=4, grad_dist=P, grad_log_policy=P, B=2, H=8, W=8,
             neighbor_mask=0x1EF, tau=0.5, horizon=16, grad_cost_out=P, status_out=P, workspace=P, workspace_bytes=BIG, stream=None)
    a.update(over)
    return a


# (the table of tests/test_soft_fields_tiled.py: the refusals are those of the fourteenth header's entry points, in the same order)
SHARED = [(dict(neighbor_mask=0x1FF), 2), (dict(neighbor_mask=0x200), 2), (dict(cost=None), 5), (dict(goal=None), 5), (dict(passable=None), 5),
          (dict(status_out=None), 5), (dict(workspace=None), 5), (dict(B=0), 1), (dict(H=0), 1), (dict(W=-1), 1), (dict(horizon=0), 1),
          (dict(horizon=-3), 1), (dict(checkpoint_every=0), 1), (dict(checkpoint_every=-2), 1),
          (dict(tau=0.0), 1), (dict(tau=-1.0), 1), (dict(tau=float("nan")), 1), (dict(tau=float("inf")), 1),
          (dict(neighbor_mask=0x010, cost=None), 2),                 # the mask is looked at first
          (dict(cost=None, B=0), 5), (dict(workspace=None, checkpoint_every=0), 5),   # a NULL before the shape
          (dict(tau=0.0, H=1024, W=1153), 1), (dict(checkpoint_every=0, H=1024, W=1153), 1),   # the shape, tau and c before the limit
          (dict(H=1024, W=1153), 2), (dict(H=1, W=1179649), 2), (dict(H=65536, W=65536), 2),
          (dict(B=(1 << 24) + 1, H=1, W=1), 2),                      # more than 2^24 tiles in the batch
          (dict(H=1024, W=1153, workspace_bytes=0), 2),              # the limit before the workspace
          (dict(workspace_bytes=0), 6), (dict(workspace=P + 8), 6)]


def _tile_sweeps(lib):
    import ctypes
    S = ctypes.c_int(-1)
    assert lib.nastar_soft_fields_tile(None, None, ctypes.addressof(S)) == 0
    return S.value


@pytest.mark.parametrize("over,rc", SHARED + [
    (dict(dist_out=None), 5), (dict(log_policy_out=None), 5), (dict(log_policy_out=None, B=0), 5),
    (dict(tape=P, tape_bytes=2 * 64 * 5 * 4 - 1), 6), (dict(tape=P + 4, tape_bytes=BIG), 6), (dict(tape=P, tape_bytes=0), 6),
    (dict(H=1024, W=1153, tape=P, tape_bytes=0), 2),               # the limit before the tape
    (dict(tape=P, tape_bytes=0, workspace_bytes=0), 6)])
def test_soft_policy_forward_tiled_refuses_bad_arguments_without_a_device(over, rc):
    from neural_astar import _native
    lib = _native.load()
    S = _tile_sweeps(lib)
    assert lib.nastar_soft_policy_forward_tiled(*_fwd(**over).values()) == rc
    assert lib.nastar_soft_policy_forward_tiled(*_fwd(**dict(dict(policy_out=P), **over)).values()) == rc
    for sweeps in (1, S):
        a = list(_fwd(**over).values())
        assert lib.nastar_soft_policy_forward_tiled_with_sweeps(*a[:-1], sweeps, a[-1]) == rc
    assert lib.nastar_last_error() == b""


def test_sweeps_per_launch_and_the_exact_workspace_size_are_checked_without_a_device():
    from neural_astar import _native
    lib = _native.load()
    S = _tile_sweeps(lib)
    a = list(_fwd().values())
    for sweeps, rc in ((0, 1), (-1, 1), (S + 1, 1)):
        assert lib.nastar_soft_policy_forward_tiled_with_sweeps(*a[:-1], sweeps, a[-1]) == rc
    bad_mask = list(_fwd(neighbor_mask=0x1FF).values())
    assert lib.nastar_soft_policy_forward_tiled_with_sweeps(*bad_mask[:-1], 0, bad_mask[-1]) == 2      # the mask first
    no_logp = list(_fwd(log_policy_out=None).values())
    assert lib.nastar_soft_policy_forward_tiled_with_sweeps(*no_logp[:-1], 0, no_logp[-1]) == 5        # a NULL before the sweeps
    too_big = list(_fwd(H=1024, W=1153).values())
    assert lib.nastar_soft_policy_forward_tiled_with_sweeps(*too_big[:-1], S + 1, too_big[-1]) == 1    # the shape before the limit
    # one byte short of what the size functions say is refused
    need = lib.nastar_soft_fields_tiled_workspace_bytes(2, 8, 8)
    assert need > 0 and lib.nastar_soft_policy_forward_tiled(*_fwd(workspace_bytes=need - 1).values()) == 6
    need = lib.nastar_soft_policy_tiled_backward_workspace_bytes(2, 8, 8, 16, 4)
    assert need > 0 and lib.nastar_soft_policy_backward_tiled(*_bwd(workspace_bytes=need - 1).values()) == 6
    assert lib.nastar_last_error() == b""


SEEDS = (dict(), dict(grad_dist=None), dict(grad_log_policy=None), dict(grad_dist=None, grad_log_policy=None))   # either may be NULL


@pytest.mark.parametrize("over,rc", SHARED + [
    (dict(tape=None), 5), (dict(grad_cost_out=None), 5),
    (dict(H=1024, W=1153, tape_bytes=0), 2),                       # the limit before the tape
    (dict(tape_bytes=2 * 64 * 5 * 4 - 1), 6), (dict(tape=P + 8), 6), (dict(horizon=20), 6), (dict(B=3), 6),
    (dict(checkpoint_every=3), 6),                                 # 16 / 3 + 1 = 6 planes: the tape of another spacing is too small
    (dict(tape_bytes=0, workspace_bytes=0), 6)])
def test_soft_policy_backward_tiled_refuses_bad_arguments_without_a_device(over, rc):
    from neural_astar import _native
    lib = _native.load()
    for seeds in SEEDS:
        assert lib.nastar_soft_policy_backward_tiled(*_bwd(**dict(seeds, **over)).values()) == rc
    assert lib.nastar_last_error() == b""


def test_null_seeds_are_not_a_refusal():
    """with a workspace one byte short the call is refused for the WORKSPACE whatever the seeds: the NULL check has let them through"""
    from neural_astar import _native
    lib = _native.load()
    need = lib.nastar_soft_policy_tiled_backward_workspace_bytes(2, 8, 8, 16, 4)
    for seeds in SEEDS:
        assert lib.nastar_soft_policy_backward_tiled(*_bwd(**dict(seeds, workspace_bytes=need - 1)).values()) == 6
        assert lib.nastar_soft_policy_backward_tiled(*_bwd(**dict(seeds, grad_cost_out=None, workspace_bytes=need - 1)).values()) == 5


# ---- 4: Python refusals before a launch; the planner methods ----------------------------------------------------------------------------------------
def test_refusals_before_a_launch_and_the_planner_methods():
    from neural_astar import ops
    from neural_astar.planner import NeuralAstar, VanillaAstar
    from neural_astar.planner.differentiable_astar import DifferentiableAstar
    assert list(inspect.signature(ops.soft_policy_tiled).parameters) == ["cost_maps", "goal_maps", "obstacles_maps", "tau", "horizon", "neighbor_mask",
                                                                         "checkpoint_every"]
    old = ["cost_maps", "goal_maps", "obstacles_maps", "opt_policies", "tau", "horizon", "neighbor_mask"]
    assert list(inspect.signature(ops.soft_policy_nll).parameters) == old          # as it was
    assert list(inspect.signature(ops.soft_policy_nll_tiled).parameters) == old + ["checkpoint_every"]
    assert list(inspect.signature(ops.soft_policy_tiled_forward).parameters) == [
        "cost_maps", "goal_maps", "obstacles_maps", "tau", "horizon", "neighbor_mask", "policies", "tape", "checkpoint_every", "sweeps_per_launch"]
    assert list(inspect.signature(ops.soft_policy_tiled_backward).parameters) == [
        "cost_maps", "goal_maps", "obstacles_maps", "tape", "grad_dists", "grad_log_policies", "tau", "horizon", "neighbor_mask", "checkpoint_every"]
    for cls in (DifferentiableAstar, VanillaAstar, NeuralAstar):
        prm = inspect.signature(cls.soft_policy_tiled).parameters
        assert prm["horizon"].default is None and prm["checkpoint_every"].default is None, cls
        assert list(prm)[-2:] == ["horizon", "checkpoint_every"], cls
        prm = inspect.signature(cls.policy_nll).parameters
        assert list(prm)[-3:] == ["horizon", "tiled", "checkpoint_every"], cls
        assert prm["tiled"].default is False and prm["checkpoint_every"].default is None and prm["horizon"].default is None, cls
    m = torch.ones(2, 1, 8, 8, requires_grad=True)
    opt = torch.zeros(2, 8, 8, 8)
    tape = torch.zeros(8, dtype=torch.uint8)
    for c in (0, -1, 1.5, True, "3", 2 ** 31):
        with pytest.raises(ValueError, match="checkpoint_every"):
            ops.soft_policy_tiled(m, m, m, 0.5, checkpoint_every=c)
        with pytest.raises(ValueError, match="checkpoint_every"):
            ops.soft_policy_nll_tiled(m, m, m, opt, 0.5, checkpoint_every=c)
        with pytest.raises(ValueError, match="checkpoint_every"):
            ops.soft_policy_tiled_forward(m, m, m, 0.5, checkpoint_every=c)
        with pytest.raises(ValueError, match="checkpoint_every"):
            ops.soft_policy_tiled_backward(m, m, m, tape, None, None, 0.5, checkpoint_every=c)
        with pytest.raises(ValueError, match="checkpoint_every"):
            DifferentiableAstar().policy_nll(m, m, m, opt, 0.5, tiled=True, checkpoint_every=c)
    for planner, args in ((DifferentiableAstar(), (m, m, m, opt, 0.5)), (VanillaAstar(), (m, m, opt, 0.5)), (NeuralAstar(), (m, m, m, opt, 0.5))):
        with pytest.raises(ValueError, match="checkpoint_every"):  # the one-workgroup field has no checkpoints
            planner.policy_nll(*args, checkpoint_every=4)
    # opt_policies is looked at before anything else could be launched: a wrong shape, a wrong device
    for wrong in (torch.zeros(2, 8, 8, 9), torch.zeros(2, 9, 8, 8), torch.zeros(3, 8, 8, 8), torch.zeros(2, 8, 64), None):
        with pytest.raises(ValueError, match="opt_policies"):
            ops.soft_policy_nll_tiled(m, m, m, wrong, 0.5)
    with pytest.raises(ValueError, match="opt_policies"):
        ops.soft_policy_nll_tiled(m, m, m, torch.zeros(2, 8, 8, 8, device="meta"), 0.5)
    for tau in (0.0, -0.5, float("nan"), float("inf"), True, None):
        with pytest.raises(ValueError, match="tau"):
            ops.soft_policy_tiled(m, m, m, tau)
        with pytest.raises(ValueError, match="tau"):
            ops.soft_policy_nll_tiled(m, m, m, opt, tau)
    for horizon in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="horizon"):
            ops.soft_policy_tiled(m, m, m, 0.5, horizon=horizon)
    with pytest.raises(ValueError, match="sweeps_per_launch"):
        ops.soft_policy_tiled_forward(m, m, m, 0.5, sweeps_per_launch=0)
    with pytest.raises(ValueError, match="neighbor_mask"):
        ops.soft_policy_tiled(m, m, m, 0.5, neighbor_mask=0x1FF)
    with pytest.raises(ValueError, match="share one"):
        ops.soft_policy_tiled(m, torch.ones(2, 1, 8, 9), m, 0.5)
    with pytest.raises(ValueError, match="grad_log_policies"):
        ops.soft_policy_tiled_backward(m, m, m, tape, None, torch.zeros(2, 8, 8, 9), 0.5)
    # tensors on the CPU: there is no CPU path, with a gradient or without
    for x in (m, m.detach()):
        with pytest.raises(RuntimeError, match="HIP device"):
            ops.soft_policy_tiled(x, x, x, 0.5)
    big = torch.ones(1, 1, 96, 136, requires_grad=True)           # above both one-workgroup limits: taken (and refused for the device only)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.soft_policy_tiled(big, big, big, 0.5)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.soft_policy_nll_tiled(big, big, big, torch.zeros(1, 8, 96, 136), 0.5)
    with pytest.raises(NotImplementedError, match="6144"):        # the one-workgroup calls refuse it as they did
        ops.soft_policy(big, big, big, 0.5)
    with pytest.raises(NotImplementedError, match="6144"):
        DifferentiableAstar().policy_nll(big, big, big, torch.zeros(1, 8, 96, 136), 0.5)
    ok = torch.ones(1, 1024, 1152)                                # the limit itself is taken
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.soft_policy_tiled(ok, ok, ok, 0.5, horizon=2)
    huge = torch.ones(1, 1, 1179649)                              # one cell more
    for call in (lambda: ops.soft_policy_tiled(huge, huge, huge, 0.5),
                 lambda: ops.soft_policy_tiled(huge.clone().requires_grad_(True), huge, huge, 0.5),
                 lambda: ops.soft_policy_nll_tiled(huge, huge, huge, torch.zeros(1, 8, 1, 1179649), 0.5),
                 lambda: ops.soft_policy_tiled_forward(huge, huge, huge, 0.5),
                 lambda: ops.soft_policy_tiled_backward(huge, huge, huge, tape, None, None, 0.5),
                 lambda: VanillaAstar().soft_policy_tiled(huge, huge, 0.5)):
        with pytest.raises(NotImplementedError, match="1179648"):
            call()
    with pytest.raises(ValueError, match="tau"):
        VanillaAstar().soft_policy_tiled(m, m, 0.0)
    with pytest.raises(ValueError, match="tau"):
        NeuralAstar().policy_nll(m, m, m, opt, -1.0, tiled=True)
    with pytest.raises(ValueError, match="tau"):
        NeuralAstar().soft_policy_tiled(m, m, m, -1.0)
    with pytest.raises(RuntimeError, match="HIP device"):
        DifferentiableAstar().policy_nll(m, m, m, opt, 0.5, tiled=True)


# ---- 5: the float32 restatement on the cases of the GPU tests -----------------------------------------------------------------------------------------
def test_the_loss_case_is_what_the_gpu_test_says_it_is():
    """two 130x140 maps, K = 97: map 1 has 27 demonstrated actions whose target has no goal within 96 moves, map 0 none; without those
    cells more than 12000 cells per map are counted"""
    cost, passable, goal = PC.loss_maps()
    opt = PC.loss_opt_policies()
    assert opt.shape == (PC.LOSS_B, 8, PC.LOSS_H, PC.LOSS_W) and (opt.sum(1) <= 1).all()
    for tau in TC.MAXENT_TAUS:
        logp, act = PO.log_policies(cost, goal, passable, tau, PC.LOSS_K)
        out = PC.shown_outside_act(opt, act)
        assert out.sum((1, 2)).tolist() == [0, 27]
        w = np.where(out[:, None], 0, opt)
        counted = (act.any(1) & (w != 0).any(1)).sum((1, 2))
        assert counted.tolist() == [13703, 12587]
        loss, dlogp = PO.nll(logp, act, w)
        assert np.isfinite(loss).all() and (loss > 0).all() and np.isfinite(dlogp).all()


def test_float32_restatement_of_the_tiled_policy_cases():
    """the float32 restatement of the VJP against float64 on exactly the cases the GPU tests hold to PTILED_RTOL: the figure that constant
    is 4 x of (TC.ABOVE: 2.681e-05; the loss case: 3.793e-05)"""
    worst = 0.0
    for H, W, B, seed, K in TC.ABOVE:
        cost, passable, goal = TC.maps(H, W, B, seed)
        for mask in TC.ABOVE_MASKS:
            for tau in SO.TAUS:
                _, act = PO.log_policies(cost, goal, passable, tau, K, mask)
                assert np.array_equal(act, PO.log_policies(cost, goal, passable, tau, K, mask, f32)[1])
                G, GL = PC.upstreams(seed, act)
                err = PC.restatement(cost, goal, passable, G, GL, tau, K, mask)
                print(f"{H}x{W} K={K} tau={tau} mask={mask:#05x}: float32 restatement of the policy gradient {err:.3e}")
                worst = max(worst, err)
    cost, passable, goal = PC.loss_maps()
    opt = PC.loss_opt_policies()
    for tau in TC.MAXENT_TAUS:
        logp, act = PO.log_policies(cost, goal, passable, tau, PC.LOSS_K)
        w = np.where(PC.shown_outside_act(opt, act)[:, None], 0, opt)
        err = PC.restatement(cost, goal, passable, None, PO.nll(logp, act, w)[1], tau, PC.LOSS_K)
        print(f"the loss case tau={tau}: float32 restatement of the gradient {err:.3e}")
        worst = max(worst, err)
    print(f"float32 restatement, the worst case: {worst:.3e}; PTILED_RTOL = {PC.PTILED_RTOL:.3e}")
    assert 0 < worst <= PC.PTILED_RTOL / 4 * 1.05
