"""GPU (-m gpu): every entry point of the field family in ``ops.py`` on the tensors real callers pass -- misaligned, sliced, multi-channel,
broadcast, transposed and row-padded inputs, non-contiguous upstream gradients (tests/field_layouts.py) -- and on costs modified in place
between forward and backward.

Two assertions per entry point, both on every output tensor:

1. the ``fresh`` call (contiguous, 16-byte aligned) against the DEFINITION: the oracle module and the rule the entry point's own GPU test
   holds it to -- equality for the exact family (``fields_grad``'s derived bound for its fp64 sums), ``SO.FWD_RTOL`` / ``SO.BWD_RTOL`` /
   ``PO.PGRAD_RTOL`` for the soft family with the infinities and the never-live zeros held exactly.  No tolerance is introduced here.
2. every other layout against the ``fresh`` call, BIT FOR BIT: the headers promise that each kernel is a pure function of the input
   values (the exact field is a unique fixed point; the soft and tiled kernels document "the same bits twice"), and a layout changes only
   which load path or which host-side copy runs.  Diagnostics that may vary (sweeps, rounds, tile visits) are not compared.

The maps come from the generators of the entry points' own GPU tests; the shapes (tests/field_layouts.py) are the smallest at which each
kernel path exists, all with an odd H*W.  tau is 0.1; the masks are Moore-8 and the directed 0x0EB.
"""
import collections
import functools

import numpy as np
import pytest
import torch

import field_layouts as FL
import field_routes_oracle as RO
import fields_grad_oracle as GO
import fields_oracle as FO
import path_masks_oracle as PMO
import soft_fields_oracle as SO
import soft_policy_oracle as PO
import test_field_routes_gpu as TR
import test_fields_gpu as TF
import test_fields_grad_gpu as TG
import test_path_masks_gpu as TP
import test_soft_fields_gpu as TS
import test_soft_policy_gpu as TSP

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
B = FL.B
TAU = 0.1
LAM, MIN_COST = 20.0, 0.25                       # the blackbox step of tests/test_path_masks_gpu.py's autograd test
CONST = -0.04                                    # the stride-0 upstream gradient: lambda * CONST = -0.8 drives most costs into the clamp
SOFT_SEEDS = {(5, 7): 4, (31, 33): 5, (65, 65): 12}   # SO.SHAPE_CASES' seeds; 65x65 is the tiled case
TILED_K, TILED_C = 24, 5                         # the soft tiled horizon and checkpoint spacing: segments of 5, 5, 5, 5 and a partial 4
EXACT_CASES = [(H, W, False) for H, W in FL.EXACT_SHAPES] + [(H, W, True) for H, W in FL.TILED_SHAPES]
PAIRS = collections.Counter()                    # (entry point, layouts) pairs run, for the figure each test prints


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


def _on(values, layout="fresh"):
    return FL.lay(values, layout, _dev())


def _same_bits(got, fresh, what):
    """every output tensor of a call in another layout has the bits of the fresh call's"""
    assert len(got) == len(fresh), what
    for k, (a, b) in enumerate(zip(got, fresh)):
        if a is None or b is None:
            assert a is None and b is None, what
            continue
        assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: output {k} is {a.dtype}{tuple(a.shape)}, the fresh call's {b.dtype}{tuple(b.shape)}"
        same = torch.equal(a.detach().contiguous().view(torch.uint8), b.detach().contiguous().view(torch.uint8))
        assert same, f"{what}: output {k} differs from the fresh call's in {int((a.detach() != b.detach()).sum())} values"


def _sweep(entry, call, values, fresh, combos, what):
    """``call(*tensors) -> tuple of tensors`` on ``values`` (three numpy maps) in every layout triple of ``combos``, against ``fresh``"""
    for combo in combos:
        got = call(*(_on(v, name) for v, name in zip(values, combo)))
        _same_bits(got, fresh, f"{entry} {what} {combo}")
        PAIRS[entry, combo] += 1
    PAIRS[entry, ("fresh",) * 3] += 1


def _leaf(values, layout):
    return _on(values, layout).requires_grad_(True)


def _grad_of(leaf, H, W):
    """the gradient autograd left on a cost leaf -> [B,H,W]; of a [B,2,H,W] leaf channel 1 must be +0.0f exactly and channel 0 is returned"""
    g = leaf.grad
    assert g is not None and tuple(g.shape) == tuple(leaf.shape), "the gradient arrives in the shape of the input"
    if leaf.ndim == 4 and leaf.shape[1] == 2:
        assert not g[:, 1].contiguous().view(torch.int32).any(), "the gradient of channel 1 is +0.0f, bit for bit"
        return g[:, 0].contiguous()
    return g.reshape(B, H, W).contiguous()


def _combos(shared):
    return FL.input_combinations(broadcast=True)[-3:] if shared else FL.input_combinations()


def _share(goal, passable):
    """the batch whose maps share map 0's goal and obstacles: what ``broadcast`` can show"""
    return tuple(np.repeat(a[:1], B, axis=0) for a in (goal, passable))


def _upstreams(G, H, W, autograd=False):
    """an upstream gradient of ``dists`` / ``paths`` in its layouts -> [(name, tensor)], the fresh one first.  ``autograd``: [B,1,H,W] each"""
    out = []
    for name in FL.GRAD_LAYOUTS:
        t = _on(G, name)
        out.append((name, t[:, None] if autograd and t.ndim == 3 else t))
    return out


def _report(test):
    print(f"{test}: {len(PAIRS)} (entry point, layouts) pairs so far, {sum(PAIRS.values())} calls")


# ---- the exact family: the field, its gradient, routes ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _exact(H, W, mask, shared=False, const=False):
    """the maps of tests/test_fields_grad_gpu.py and the definition on them -> (cost, goal, passable, G, FO.fields, GO.field_grads)"""
    cost, goal, passable, G = TG._case(H, W)
    if shared:
        goal, passable = _share(goal, passable)
    if const:
        G = np.full_like(G, CONST)
    refs = GO.field_grads(cost, goal, passable, G, mask)
    assert all(r.status == 0 for r in refs), "U(0.5, 1.5) costs have no plateau at these sizes"
    return cost, goal, passable, G, FO.fields(cost, goal, passable, mask), refs


def _field_call(ops, tiled_entry, mask, **how):
    if tiled_entry:
        return lambda c, g, p: tuple(ops.cost_to_go_tiled(c, g, p, neighbor_mask=mask, **how)[0])
    return lambda c, g, p: tuple(ops.cost_to_go(c, g, p, neighbor_mask=mask, **how))


@pytest.mark.parametrize("shared", [False, True], ids=["", "shared"])
@pytest.mark.parametrize("mask", FL.MASKS, ids=hex)
@pytest.mark.parametrize("H,W,tiled", EXACT_CASES)
def test_cost_to_go(H, W, tiled, mask, shared):
    from neural_astar import ops
    cost, goal, passable, G, want, refs = _exact(H, W, mask, shared)
    what = f"{H}x{W} {mask:#x}"
    entries = {"cost_to_go_tiled": _field_call(ops, True, mask)} if tiled else \
              {"cost_to_go": _field_call(ops, False, mask), "cost_to_go(tiled=True)": _field_call(ops, False, mask, tiled=True)}
    for entry, call in entries.items():
        fresh = call(_on(cost), _on(goal), _on(passable))
        TF._same(ops.FieldOutput(*fresh), want, f"{entry} {what}")
        _sweep(entry, call, (cost, goal, passable), fresh, _combos(shared), what)

    # differentiable=True: the same outputs, and the gradient that autograd leaves on the cost leaf
    entry = "cost_to_go_tiled(differentiable=True)" if tiled else "cost_to_go(differentiable=True)"

    def through(c, g, p, up=None):
        leaf = c.requires_grad_(True)
        out = _field_call(ops, tiled, mask, differentiable=True)(leaf, g, p)
        assert out[0].requires_grad
        out[0].backward(_on(G)[:, None] if up is None else up)
        return out + (_grad_of(leaf, H, W),)

    fresh = through(_on(cost), _on(goal), _on(passable))
    TF._same(ops.FieldOutput(*(t.detach() for t in fresh[:3])), want, f"{entry} {what}")
    TG._close(fresh[3].cpu().numpy(), refs, G, f"{entry} {what}")
    _sweep(entry, through, (cost, goal, passable), fresh, _combos(shared), what)
    if not shared:
        for name, up in _upstreams(G, H, W, autograd=True)[1:]:
            _same_bits(through(_on(cost), _on(goal), _on(passable), up), fresh, f"{entry} {what} upstream {name}")
            PAIRS[entry, ("upstream", name)] += 1
        flat = through(_on(cost), _on(goal), _on(passable), torch.full((B, 1, H, W), CONST, device=_dev()))
        TG._close(flat[3].cpu().numpy(), _exact(H, W, mask, const=True)[5], np.full_like(G, CONST), f"{entry} {what} constant upstream")
        _same_bits(through(_on(cost), _on(goal), _on(passable), FL.stride0(CONST, B, H, W, _dev())), flat, f"{entry} {what} upstream stride0")
        PAIRS[entry, ("upstream", "stride0")] += 1
    _report("cost_to_go")


@pytest.mark.parametrize("shared", [False, True], ids=["", "shared"])
@pytest.mark.parametrize("mask", FL.MASKS, ids=hex)
@pytest.mark.parametrize("H,W,tiled", EXACT_CASES)
def test_fields_backward(H, W, tiled, mask, shared):
    from neural_astar import ops
    cost, goal, passable, G, want, refs = _exact(H, W, mask, shared)
    dists = want[0]
    entry, what = "fields_backward_tiled" if tiled else "fields_backward", f"{H}x{W} {mask:#x}"
    raw = ops.fields_backward_tiled if tiled else ops.fields_backward

    def call(d, g, p, up=None):
        return tuple(raw(d, g, p, _on(G) if up is None else up, neighbor_mask=mask)[:2])

    fresh = call(_on(dists), _on(goal), _on(passable))
    TG._close(fresh[0].cpu().numpy(), refs, G, f"{entry} {what}")
    assert fresh[1].tolist() == [0] * B
    _sweep(entry, call, (dists, goal, passable), fresh, _combos(shared), what)
    if not shared:
        for name, up in _upstreams(G, H, W)[1:]:
            _same_bits(call(_on(dists), _on(goal), _on(passable), up), fresh, f"{entry} {what} upstream {name}")
            PAIRS[entry, ("upstream", name)] += 1
        flat = call(_on(dists), _on(goal), _on(passable), torch.full((B, H, W), CONST, device=_dev()))
        TG._close(flat[0].cpu().numpy(), _exact(H, W, mask, const=True)[5], np.full_like(G, CONST), f"{entry} {what} constant upstream")
        _same_bits(call(_on(dists), _on(goal), _on(passable), FL.stride0(CONST, B, H, W, _dev())), flat, f"{entry} {what} upstream stride0")
        # every input and the upstream gradient in another layout at once
        _same_bits(call(_on(dists, "tail"), _on(goal, "rowpad"), _on(passable, "channel0"), _on(G, "transposed")), fresh, f"{entry} {what} all at once")
        PAIRS[entry, ("upstream", "stride0")] += 1
    _report("fields_backward")


@pytest.mark.parametrize("shared", [False, True], ids=["", "shared"])
@pytest.mark.parametrize("mask", FL.MASKS, ids=hex)
@pytest.mark.parametrize("H,W", sorted(set(FL.EXACT_SHAPES + FL.TILED_SHAPES)))
def test_field_routes(H, W, mask, shared):
    from neural_astar import ops
    cost, goal, passable, _, want, _ = _exact(H, W, mask, shared)
    dists = want[0]
    starts = TR._starts(dists, goal, passable, 6)
    what = f"{H}x{W} {mask:#x}"

    starts_t = torch.from_numpy(starts).to(_dev())
    call = lambda d, g, p: tuple(ops.field_routes(d, g, p, starts_t, neighbor_mask=mask))  # noqa: E731
    fresh = call(_on(dists), _on(goal), _on(passable))
    ref = RO.batch(dists, goal, passable, starts, mask)
    TR._same(tuple(t.cpu().numpy() for t in fresh), ref, f"field_routes {what}")
    assert (ref[3] == 0).any(), "some query was meant to have a route"
    _sweep("field_routes", call, (dists, goal, passable), fresh, _combos(shared), what)
    _report("field_routes")


# ---- the exact family: path masks and their blackbox gradient --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _paths(H, W, mask, shared=False, const=False):
    """the maps, starts and targets of tests/test_path_masks_gpu.py and the definition on them"""
    cost, goal, passable = TP._maps(H, W)
    if shared:
        goal, passable = _share(goal, passable)
    dist = FO.fields(cost, goal, passable, mask)[0].reshape(B, -1)
    starts = np.argmax(np.where(np.isfinite(dist), dist, -1), axis=1).astype(np.int32)       # the longest chase (``TP._starts``)
    want = PMO.batch(cost, goal, passable, starts, mask)
    assert (want[2] == 0).all(), "every map was meant to be solved"
    other = (0.25 + np.random.default_rng([9, H, W, B]).random(cost.shape)).astype(f32)     # (``TP._targets``)
    grad = (1 - 2 * PMO.batch(other, goal, passable, starts, mask)[0]).astype(f32)
    if const:
        grad = np.full_like(grad, CONST)
    want_grad, want_st, changed, clamped = PMO.batch_backward(cost, goal, passable, starts, grad, LAM, MIN_COST, mask)
    assert (want_st == 0).all() and clamped.any(), "the clamp was meant to bind"
    return cost, goal, passable, starts, grad, want, want_grad, bool(changed.any())


@pytest.mark.parametrize("shared", [False, True], ids=["", "shared"])
@pytest.mark.parametrize("mask", FL.MASKS, ids=hex)
@pytest.mark.parametrize("H,W,tiled", EXACT_CASES)
def test_path_masks(H, W, tiled, mask, shared):
    from neural_astar import ops
    cost, goal, passable, starts, grad, want, want_grad, changed = _paths(H, W, mask, shared)
    if not shared and H > 1:
        assert changed, "the perturbed path was meant to differ from the forward one on some map"
    sfx, what = "_tiled" if tiled else "", f"{H}x{W} {mask:#x}"
    forward = ops.path_masks_tiled if tiled else ops.path_masks
    backward = ops.path_masks_tiled_backward if tiled else ops.path_masks_backward
    layer = ops.shortest_paths_tiled if tiled else ops.shortest_paths
    s = torch.from_numpy(starts).to(_dev())
    numpy3 = lambda out: (out[0][:, 0].detach().cpu().numpy(), out[1].cpu().numpy(), out[2].cpu().numpy())  # noqa: E731

    call = lambda c, g, p: tuple(forward(c, g, p, s, neighbor_mask=mask))  # noqa: E731
    fresh = call(_on(cost), _on(goal), _on(passable))
    TP._same(numpy3(fresh), want, f"path_masks{sfx} {what}")
    _sweep(f"path_masks{sfx}", call, (cost, goal, passable), fresh, _combos(shared), what)
    paths_np, status = fresh[0][:, 0].cpu().numpy(), fresh[2]

    def raw(c, g, p, up=None, fwd=None):
        return tuple(backward(c, g, p, s, _on(grad) if up is None else up, fresh[0] if fwd is None else fwd, status, LAM, MIN_COST, neighbor_mask=mask))

    fresh_b = raw(_on(cost), _on(goal), _on(passable))
    TP._same_grad(fresh_b[0].cpu().numpy(), want_grad, f"path_masks{sfx}_backward {what}")
    assert fresh_b[1].tolist() == [0] * B
    _sweep(f"path_masks{sfx}_backward", raw, (cost, goal, passable), fresh_b, _combos(shared), what)

    def through(c, g, p, up=None):
        leaf = c.requires_grad_(True)
        out = tuple(layer(leaf, s, g, p, neighbor_mask=mask, lambda_=LAM, min_cost=MIN_COST))
        assert out[0].requires_grad
        out[0].backward(_on(grad)[:, None] if up is None else up)
        return out + (_grad_of(leaf, H, W),)

    fresh_l = through(_on(cost), _on(goal), _on(passable))
    TP._same(numpy3(fresh_l), want, f"shortest_paths{sfx} {what}")
    TP._same_grad(fresh_l[3].cpu().numpy(), want_grad, f"shortest_paths{sfx} {what}")
    _sweep(f"shortest_paths{sfx}", through, (cost, goal, passable), fresh_l, _combos(shared), what)
    if not shared:
        flat_want = _paths(H, W, mask, const=True)[6]
        for name, up in _upstreams(grad, H, W)[1:]:
            _same_bits(raw(_on(cost), _on(goal), _on(passable), up), fresh_b, f"path_masks{sfx}_backward {what} upstream {name}")
            PAIRS[f"path_masks{sfx}_backward", ("upstream", name)] += 1
        for name in ("transposed", "rowpad", "shift1"):           # ``paths_fwd`` too, alone and with the vec flag's other pointers moved
            _same_bits(raw(_on(cost), _on(goal), _on(passable), fwd=_on(paths_np, name)), fresh_b, f"path_masks{sfx}_backward {what} paths_fwd {name}")
            PAIRS[f"path_masks{sfx}_backward", ("paths_fwd", name)] += 1
        _same_bits(raw(_on(cost, "shift1"), _on(goal, "tail"), _on(passable, "channel0"), _on(grad, "transposed"), _on(paths_np, "transposed")),
                   fresh_b, f"path_masks{sfx}_backward {what} all at once")
        flat = raw(_on(cost), _on(goal), _on(passable), torch.full((B, H, W), CONST, device=_dev()))
        TP._same_grad(flat[0].cpu().numpy(), flat_want, f"path_masks{sfx}_backward {what} constant upstream")
        _same_bits(raw(_on(cost), _on(goal), _on(passable), FL.stride0(CONST, B, H, W, _dev())), flat, f"path_masks{sfx}_backward {what} upstream stride0")
        PAIRS[f"path_masks{sfx}_backward", ("upstream", "stride0")] += 1
        for name, up in _upstreams(grad, H, W, autograd=True)[1:]:
            _same_bits(through(_on(cost), _on(goal), _on(passable), up), fresh_l, f"shortest_paths{sfx} {what} upstream {name}")
            PAIRS[f"shortest_paths{sfx}", ("upstream", name)] += 1
        got = through(_on(cost), _on(goal), _on(passable), FL.stride0(CONST, B, H, W, _dev()))
        TP._same_grad(got[3].cpu().numpy(), flat_want, f"shortest_paths{sfx} {what} upstream stride0")
        PAIRS[f"shortest_paths{sfx}", ("upstream", "stride0")] += 1
    _report("path_masks")


# ---- the soft family ---------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _soft(H, W, shared=False):
    cost, passable, goal = SO.random_maps(SOFT_SEEDS[H, W], B, H, W)
    if shared:
        goal, passable = _share(goal, passable)
    return cost, goal, passable


def _soft_calls(ops, tiled, H, W, mask):
    """-> (K, forward(c, g, p) -> (dists, policies, status, tape), backward(c, g, p, tape, up) -> (grad, status), layer, nll)"""
    if tiled:
        K = TILED_K
        return (K,
                lambda c, g, p: _flat(ops.soft_fields_tiled_forward(c, g, p, TAU, K, mask, policies=True, tape=True, checkpoint_every=TILED_C)),
                lambda c, g, p, tape, up: tuple(ops.soft_fields_tiled_backward(c, g, p, tape, up, TAU, K, mask, checkpoint_every=TILED_C)),
                lambda c, g, p: ops.soft_cost_to_go_tiled(c, g, p, TAU, K, mask, policies=True, differentiable=True, checkpoint_every=TILED_C),
                lambda c, s, g, p, t: ops.maxent_path_nll_tiled(c, s, g, p, t, TAU, K, mask, checkpoint_every=TILED_C))
    K = 2 * (H + W)
    return (K,
            lambda c, g, p: _flat(ops.soft_fields_forward(c, g, p, TAU, K, mask, policies=True, tape=True)),
            lambda c, g, p, tape, up: tuple(ops.soft_fields_backward(c, g, p, tape, up, TAU, K, mask)),
            lambda c, g, p: ops.soft_cost_to_go(c, g, p, TAU, K, mask, policies=True, differentiable=True),
            lambda c, s, g, p, t: ops.maxent_path_nll(c, s, g, p, t, TAU, K, mask))


def _flat(out_and_tape):
    out, tape = out_and_tape
    return tuple(out) + (tape,)


@pytest.mark.parametrize("shared", [False, True], ids=["", "shared"])
@pytest.mark.parametrize("mask", FL.MASKS, ids=hex)
@pytest.mark.parametrize("H,W,tiled", [(H, W, False) for H, W in FL.SOFT_SHAPES] + [(H, W, True) for H, W in FL.SOFT_TILED_SHAPES])
def test_soft_fields(H, W, tiled, mask, shared):
    from neural_astar import ops
    cost, goal, passable = _soft(H, W, shared)
    K, forward, backward, layer, _ = _soft_calls(ops, tiled, H, W, mask)
    sfx, what = "_tiled" if tiled else "", f"{H}x{W} K={K} {mask:#x}"
    fresh = forward(_on(cost), _on(goal), _on(passable))
    ref_d = TS._check_forward(ops.SoftFieldOutput(*fresh[:3]), cost, passable, goal, TAU, K, mask, f"soft_fields{sfx}_forward {what}")
    _sweep(f"soft_fields{sfx}_forward", forward, (cost, goal, passable), fresh, _combos(shared), what)
    live = (passable != 0) & (goal == 0) & np.isfinite(ref_d)
    assert live.any()
    G = TS._upstream(SOFT_SEEDS[H, W], live).astype(f32)          # a NaN on every cell that is not live at the horizon
    tape = fresh[3]

    def raw(c, g, p, up=None):
        return backward(c, g, p, tape, _on(G) if up is None else up)

    fresh_b = raw(_on(cost), _on(goal), _on(passable))
    TS._check_backward(fresh_b[0], cost, passable, goal, G, TAU, K, mask, f"soft_fields{sfx}_backward {what}")
    assert fresh_b[1].tolist() == [0] * B
    _sweep(f"soft_fields{sfx}_backward", raw, (cost, goal, passable), fresh_b, _combos(shared), what)

    def through(c, g, p, up=None):
        leaf = c.requires_grad_(True)
        out = tuple(layer(leaf, g, p))
        assert out[0].requires_grad
        out[0].backward(_on(G)[:, None] if up is None else up)
        return out + (_grad_of(leaf, H, W),)

    entry = f"soft_cost_to_go{sfx}"
    fresh_l = through(_on(cost), _on(goal), _on(passable))
    _same_bits(fresh_l[:3], fresh[:3], f"{entry} {what}: the raw forward's outputs")
    _same_bits(fresh_l[3:], fresh_b[:1], f"{entry} {what}: the raw backward's gradient")
    _sweep(entry, through, (cost, goal, passable), fresh_l, _combos(shared), what)
    if not shared:
        for name, up in _upstreams(G, H, W)[1:]:
            _same_bits(raw(_on(cost), _on(goal), _on(passable), up), fresh_b, f"soft_fields{sfx}_backward {what} upstream {name}")
            PAIRS[f"soft_fields{sfx}_backward", ("upstream", name)] += 1
        for name, up in _upstreams(G, H, W, autograd=True)[1:]:
            _same_bits(through(_on(cost), _on(goal), _on(passable), up), fresh_l, f"{entry} {what} upstream {name}")
            PAIRS[entry, ("upstream", name)] += 1
        flat = raw(_on(cost), _on(goal), _on(passable), torch.full((B, H, W), CONST, device=_dev()))
        TS._check_backward(flat[0], cost, passable, goal, np.full_like(G, CONST), TAU, K, mask, f"soft_fields{sfx}_backward {what} constant upstream")
        _same_bits(raw(_on(cost), _on(goal), _on(passable), FL.stride0(CONST, B, H, W, _dev())), flat, f"soft_fields{sfx}_backward {what} stride0")
        _same_bits(through(_on(cost), _on(goal), _on(passable), FL.stride0(CONST, B, H, W, _dev()))[3:], flat[:1], f"{entry} {what} stride0")
        _same_bits(raw(_on(cost, "tail"), _on(goal, "rowpad"), _on(passable, "channel0"), _on(G, "transposed")), fresh_b, f"soft_fields{sfx}_backward {what} all at once")
        PAIRS[f"soft_fields{sfx}_backward", ("upstream", "stride0")] += 1
        PAIRS[entry, ("upstream", "stride0")] += 1
    _report("soft_fields")


@functools.lru_cache(maxsize=None)
def _demonstrations(H, W, mask, shared, K):
    """per map a start at most 8 moves (and fewer than K) from the goal and the exact shortest path from it, as the demonstration"""
    cost, goal, passable = _soft(H, W, shared)
    start = np.zeros_like(goal)
    for b in range(B):
        far = SO.hops(goal[b], passable[b], mask)
        start[b][tuple(np.argwhere(far == min(int(far.max()), 8, K - 1))[0])] = 1
    demo, _, st = PMO.batch(cost, goal, passable, [PMO.start_index(start[b]) for b in range(B)], mask)
    assert (st == 0).all()
    return start, demo


@pytest.mark.parametrize("shared", [False, True], ids=["", "shared"])
@pytest.mark.parametrize("mask", FL.MASKS, ids=hex)
@pytest.mark.parametrize("H,W,tiled", [(H, W, False) for H, W in FL.SOFT_SHAPES] + [(H, W, True) for H, W in FL.SOFT_TILED_SHAPES])
def test_maxent_path_nll(H, W, tiled, mask, shared):
    from neural_astar import ops
    cost, goal, passable = _soft(H, W, shared)
    K, _, _, _, nll = _soft_calls(ops, tiled, H, W, mask)
    start, demo = _demonstrations(H, W, mask, shared, K)
    entry, what = "maxent_path_nll_tiled" if tiled else "maxent_path_nll", f"{H}x{W} K={K} {mask:#x}"

    def through(c, g, p, s="fresh", t="fresh"):
        leaf = c.requires_grad_(True)
        loss = nll(leaf, _on(start, s), g, p, _on(demo, t))
        assert tuple(loss.shape) == (B,) and loss.requires_grad
        loss.sum().backward()
        return loss, _grad_of(leaf, H, W)

    fresh = through(_on(cost), _on(goal), _on(passable))
    # the rule of tests/test_soft_fields_gpu.py::test_maxent_path_nll_and_its_gradient
    leaves = demo.astype(f64) * (goal == 0)
    paid = (cost.astype(f64) * leaves).sum((1, 2))
    V = SO.soft_fields(cost, goal, passable, TAU, K, mask)[0]
    ref = (paid - np.where(start != 0, V, 0.0).sum((1, 2))) / TAU
    tol = (K * 2.0 ** -23 * paid.max() + SO.FWD_RTOL * np.abs(V[np.isfinite(V)]).max()) / TAU
    got = fresh[0].detach().cpu().numpy().astype(f64)
    print(f"{entry} {what}: nll {got}, against the definition {np.abs(got - ref).max():.3e} (tol {tol:.3e})")
    assert (got >= -tol).all() and np.abs(got - ref).max() <= tol
    visits = SO.soft_field_grads(cost, goal, passable, (start != 0).astype(f64), TAU, K, mask)[0]
    err = np.abs(fresh[1].cpu().numpy() - (leaves - visits) / TAU).max() / (np.abs(visits).max() / TAU)
    print(f"{entry} {what}: gradient rel err {err:.3e}")
    assert err <= SO.BWD_RTOL
    _sweep(entry, through, (cost, goal, passable), fresh, _combos(shared), what)
    if not shared:
        for s, t in (("channel0", "fresh"), ("fresh", "channel0"), ("transposed", "rowpad"), ("tail", "shift1")):
            _same_bits(through(_on(cost), _on(goal), _on(passable), s, t), fresh, f"{entry} {what} start {s}, demonstration {t}")
            PAIRS[entry, ("start", s, "demonstration", t)] += 1
    _report("maxent_path_nll")


@pytest.mark.parametrize("shared", [False, True], ids=["", "shared"])
@pytest.mark.parametrize("mask", FL.MASKS, ids=hex)
@pytest.mark.parametrize("H,W", FL.SOFT_SHAPES)
def test_soft_policy(H, W, mask, shared):
    from neural_astar import ops
    cost, goal, passable = _soft(H, W, shared)
    K, what = 2 * (H + W), f"{H}x{W} {mask:#x}"
    forward = lambda c, g, p: _flat(ops.soft_policy_forward(c, g, p, TAU, K, mask, policies=True, tape=True))  # noqa: E731
    fresh = forward(_on(cost), _on(goal), _on(passable))
    out = ops.SoftPolicyOutput(*fresh[:4])
    TS._check_forward(ops.SoftFieldOutput(out.dists, out.policies, out.status), cost, passable, goal, TAU, K, mask, f"soft_policy_forward {what}")
    _, act = TSP._check_log_policy(out, cost, passable, goal, TAU, K, mask, f"soft_policy_forward {what}")
    _sweep("soft_policy_forward", forward, (cost, goal, passable), fresh, _combos(shared), what)
    seed = SOFT_SEEDS[H, W]
    GL = PO.upstream(seed, act).astype(f32)                       # a NaN on every entry outside (live at K, Act)
    G = np.where(act.any(1), np.random.default_rng(seed + 100).standard_normal((B, H, W)), np.nan).astype(f32)
    ref, ever = PO.soft_policy_grads(cost, goal, passable, G, GL, TAU, K, mask)
    tape = fresh[4]

    def raw(c, g, p, up=None, upl=None):
        return tuple(ops.soft_policy_backward(c, g, p, tape, _on(G) if up is None else up, _on(GL) if upl is None else upl, TAU, K, mask))

    fresh_b = raw(_on(cost), _on(goal), _on(passable))
    TSP._check_grad(fresh_b[0], ref, ever, f"soft_policy_backward {what}")
    assert fresh_b[1].tolist() == [0] * B
    _sweep("soft_policy_backward", raw, (cost, goal, passable), fresh_b, _combos(shared), what)

    def through(c, g, p, up=None, upl=None):
        leaf = c.requires_grad_(True)
        o = ops.soft_policy(leaf, g, p, TAU, K, mask)
        assert o.dists.requires_grad and o.log_policies.requires_grad
        torch.autograd.backward([o.dists, o.log_policies], [_on(G)[:, None] if up is None else up, _on(GL) if upl is None else upl])
        return tuple(o) + (_grad_of(leaf, H, W),)

    fresh_l = through(_on(cost), _on(goal), _on(passable))
    _same_bits(fresh_l[:4], fresh[:4], f"soft_policy {what}: the raw forward's outputs")
    _same_bits(fresh_l[4:], fresh_b[:1], f"soft_policy {what}: the raw backward's gradient")
    _sweep("soft_policy", through, (cost, goal, passable), fresh_l, _combos(shared), what)
    if not shared:
        for name in FL.POLICY_GRAD_LAYOUTS[1:]:
            _same_bits(raw(_on(cost), _on(goal), _on(passable), upl=_on(GL, name)), fresh_b, f"soft_policy_backward {what} grad_log_policies {name}")
            _same_bits(through(_on(cost), _on(goal), _on(passable), upl=_on(GL, name)), fresh_l, f"soft_policy {what} grad_log_policies {name}")
            PAIRS["soft_policy_backward", ("grad_log_policies", name)] += 1
            PAIRS["soft_policy", ("grad_log_policies", name)] += 1
        for name, up in _upstreams(G, H, W)[1:]:
            _same_bits(raw(_on(cost), _on(goal), _on(passable), up, _on(GL, "permuted")), fresh_b, f"soft_policy_backward {what} upstream {name}, permuted")
            PAIRS["soft_policy_backward", ("upstream", name)] += 1
        flat_ref, flat_ever = PO.soft_policy_grads(cost, goal, passable, np.full_like(G, CONST), GL, TAU, K, mask)
        flat = raw(_on(cost), _on(goal), _on(passable), torch.full((B, H, W), CONST, device=_dev()))
        TSP._check_grad(flat[0], flat_ref, flat_ever, f"soft_policy_backward {what} constant upstream")
        _same_bits(raw(_on(cost), _on(goal), _on(passable), FL.stride0(CONST, B, H, W, _dev()), _on(GL, "rowpad")), flat, f"soft_policy_backward {what} stride0")
        _same_bits(through(_on(cost), _on(goal), _on(passable), FL.stride0(CONST, B, H, W, _dev()), _on(GL, "permuted"))[4:], flat[:1], f"soft_policy {what} stride0")
        PAIRS["soft_policy_backward", ("upstream", "stride0")] += 1
        PAIRS["soft_policy", ("upstream", "stride0")] += 1
    _report("soft_policy")


@pytest.mark.parametrize("shared", [False, True], ids=["", "shared"])
@pytest.mark.parametrize("mask", FL.MASKS, ids=hex)
@pytest.mark.parametrize("H,W", FL.SOFT_SHAPES)
def test_soft_policy_nll(H, W, mask, shared):
    from neural_astar import ops
    cost, goal, passable = _soft(H, W, shared)
    K, what = 2 * (H + W), f"{H}x{W} {mask:#x}"
    w = FO.fields(cost, goal, passable, mask)[1]                  # the optimal action of every cell, the dataset's order
    assert w.shape == (B, 8, H, W) and w.sum() > B

    def through(c, g, p, opt="fresh"):
        leaf = c.requires_grad_(True)
        loss = ops.soft_policy_nll(leaf, g, p, _on(w, opt), TAU, K, mask)
        assert tuple(loss.shape) == (B,) and loss.requires_grad
        loss.sum().backward()
        return loss, _grad_of(leaf, H, W)

    fresh = through(_on(cost), _on(goal), _on(passable))
    # the rule of tests/test_soft_policy_gpu.py::test_soft_policy_nll_and_its_gradient
    logp, act = PO.log_policies(cost, goal, passable, TAU, K, mask)
    ref, dlogp = PO.nll(logp, act, w)
    V = SO.soft_fields(cost, goal, passable, TAU, K, mask)[0]
    tol = 2 * SO.FWD_RTOL * np.abs(V[np.isfinite(V)]).max() / TAU + 16 * TSP.EPS * (1 + np.abs(logp[(w != 0) & act]).max())
    want, ever = PO.soft_policy_grads(cost, goal, passable, None, dlogp, TAU, K, mask)

    def definition(result, what):
        got = result[0].detach().cpu().numpy().astype(f64)
        print(f"soft_policy_nll {what}: nll {got}, against the definition {np.abs(got - ref).max():.3e} (tol {tol:.3e})")
        assert (got > 0).all() and np.abs(got - ref).max() <= tol
        TSP._check_grad(result[1], want, ever, f"soft_policy_nll {what}")

    definition(fresh, what)
    _sweep("soft_policy_nll", through, (cost, goal, passable), fresh, _combos(shared), what)
    if not shared:
        # ``opt_policies`` is no kernel's input: the loss is a torch sum over it, whose order follows its strides -- the definition's rule,
        # not the fresh call's bits
        for name in FL.POLICY_GRAD_LAYOUTS[1:]:
            definition(through(_on(cost), _on(goal), _on(passable), name), f"{what} opt_policies {name}")
            PAIRS["soft_policy_nll", ("opt_policies", name)] += 1
    _report("soft_policy_nll")


# ---- a cost modified in place between forward and backward -----------------------------------------------------------------------------------------------------
INPLACE = "modified by an inplace operation"


def _inplace_cases():
    """(name, H, W, reads the cost in its backward, saves dists): one-workgroup entries at 5x7 and 65x65, the tiled ones at 65x65 and 5x7"""
    out = []
    for H, W in ((5, 7), (65, 65)):
        out += [("cost_to_go", H, W, False, True), ("cost_to_go_tiled", H, W, False, True),
                ("shortest_paths", H, W, True, False), ("shortest_paths_tiled", H, W, True, False),
                ("soft_cost_to_go", H, W, True, True), ("soft_cost_to_go_tiled", H, W, True, True),
                ("maxent_path_nll", H, W, True, False), ("maxent_path_nll_tiled", H, W, True, False),
                ("soft_policy", H, W, True, False), ("soft_policy_nll", H, W, True, False)]
    return out


def _inplace_run(name, H, W, layout):
    """-> ``run(touch) -> gradient on the leaf [B,H,W]``: forward on ``c = leaf * 1.0``, then ``touch(c, dists or None)``, then backward"""
    from neural_astar import ops
    mask = FL.MASKS[0]
    soft = name.startswith(("soft", "maxent"))
    if soft:
        cost, goal, passable = _soft(H, W)
        K = TILED_K if (H, W) == (65, 65) else 2 * (H + W)
    elif name.startswith("shortest"):
        cost, goal, passable, starts, up_np = _paths(H, W, mask)[:5]
    else:
        cost, goal, passable, up_np = _exact(H, W, mask)[:4]
    g, p = _on(goal), _on(passable)

    def run(touch):
        leaf = _leaf(cost, layout)
        c = leaf * 1.0
        dists = None
        if name in ("cost_to_go", "cost_to_go_tiled"):
            out = ops.cost_to_go(c, g, p, differentiable=True) if name == "cost_to_go" else ops.cost_to_go_tiled(c, g, p, differentiable=True)[0]
            dists = head = out.dists
            up = _on(up_np)[:, None]
        elif name in ("shortest_paths", "shortest_paths_tiled"):
            out = getattr(ops, name)(c, torch.from_numpy(starts).to(_dev()), g, p, lambda_=LAM, min_cost=MIN_COST)
            head, up = out.paths, _on(up_np)[:, None]
        elif name in ("soft_cost_to_go", "soft_cost_to_go_tiled"):
            extra = {"checkpoint_every": TILED_C} if name.endswith("tiled") else {}
            dists = head = getattr(ops, name)(c, g, p, TAU, K, differentiable=True, **extra).dists
            up = torch.where(torch.isfinite(head.detach()), 1.0, 0.0)
        elif name in ("maxent_path_nll", "maxent_path_nll_tiled"):
            start, demo = _demonstrations(H, W, mask, False, K)
            extra = {"checkpoint_every": TILED_C} if name.endswith("tiled") else {}
            head, up = getattr(ops, name)(c, _on(start), g, p, _on(demo), TAU, K, **extra), torch.ones(B, device=_dev())
        elif name == "soft_policy":
            out = ops.soft_policy(c, g, p, TAU, K)
            head, up = out.log_policies, torch.where(torch.isfinite(out.log_policies.detach()), 1.0, 0.0)
        else:
            # the optimal actions, less those the horizon gives probability 0 (a cheapest route of more than K moves): the definition's verdict
            w = FO.fields(cost, goal, passable, mask)[1] * PO.log_policies(cost, goal, passable, TAU, K, mask)[1]
            head, up = ops.soft_policy_nll(c, g, p, _on(w), TAU, K), torch.ones(B, device=_dev())
        assert head.requires_grad
        touch(c, dists)
        head.backward(up)
        return _grad_of(leaf, H, W)

    return run


@pytest.mark.parametrize("layout", ["fresh", "channel0"])
@pytest.mark.parametrize("name,H,W,reads_cost,saves_dists", _inplace_cases(), ids=lambda v: str(v))
def test_cost_modified_in_place_between_forward_and_backward(name, H, W, reads_cost, saves_dists, layout):
    """a node whose backward reads the cost again must refuse to run on a cost that has changed since (autograd's version check on a SAVED
    tensor); the exact field's backward reads ``dists`` alone, so its gradient is that of the untouched run, bit for bit"""
    run = _inplace_run(name, H, W, layout)
    untouched = run(lambda c, d: None)
    assert bool(torch.isfinite(untouched).all()) and (bool(untouched.any()) or name.startswith("shortest"))
    if reads_cost:
        with pytest.raises(RuntimeError, match=INPLACE):
            run(lambda c, d: c.mul_(2))
    else:
        _same_bits((run(lambda c, d: c.mul_(2)),), (untouched,), f"{name} {H}x{W} {layout}: the cost doubled in place after the forward")
    if saves_dists:
        with pytest.raises(RuntimeError, match=INPLACE):
            run(lambda c, d: d.mul_(2))
    PAIRS[name, ("in place", layout)] += 1
