"""The eval-mode CNNDownSize encoder on the f32-input MFMA (csrc/nastar_encoder_downsize.hip.h, launched by
nastar_encoder_cnn_downsize_forward in csrc/nastar_encoder_capi.hip, wrapped by encoder_hip.HipCnnDownSizeEncoder), layer by layer at the
edges of its 2-row x 16-column output tile, against the float64 oracle of tests/downsize_oracle.py.

Every call to the C entry gets a cost_out one image longer than B (pre-filled with -7: the extra image must survive), a workspace 4 KiB
longer than the workspace_bytes it is told (the tail must survive) and a workspace body of 0xFF bytes (fp32 NaN: a read of anything the
launch did not write poisons what follows; no level may hold a NaN).  The prep tensor and every pooled level are read back from the
workspace at the offsets include/nastar.h documents (downsize_oracle.levels).

A  bit-exact levels: integer-valued operands (downsize_oracle.exact_operands) for which fp32 accumulation is exact in any order, the
   precondition asserted before the launch.  Every stored level is torch.equal to the oracle's; the cost map, whose pre-activation is
   exact, is within 1e-5 * max(1, final_mul) of the float64 sigmoid (what is measured is __expf).  Shapes, smallest first:
     m    depth 1   2 x 2    -> 1x1              B 3   CIN 2 first block (C = 1 padded), 1-pixel final map, one tile larger than the image
     m+   depth 1   6 x 34   -> 3x17             B 2   odd final rows, final seam 16|1, first block 3 column tiles, the last 2 wide
     rgb  depth 2   8 x 72   -> 4x36 -> 2x18     B 2   CIN 4 with a zero channel, hidden seam 32|4, final seam 16|2
     rgb+ depth 3   24 x 40  -> 12x20, 6x10, 3x5 B 37  tiles_x != tiles_y at every level under a large B (batch decode), levels below 16 wide
     m+   depth 4   16 x 16  -> 8, 4, 2 -> 1x1   B 2   all four hidden instantiations, <256,32,final> on one pixel, a 2-row level
     m+   depth 4   32 x 48  -> ... -> 2x3       B 1   B = 1
     rgb+ depth 3   96 x 96  -> ... -> 12x12     B 2   the WarCraft geometry, once
B  batch independence: image b alone has the bits it has inside the batch, on the cost map and on every level.
C  ordinary numbers through the wrapper against the torch module in float64 on the CPU, bound 1e-5 * max(1, const).
D  the wrapper's weight cache and cached workspace.
E  the start + goal channel of the prep tensor equals F.interpolate(mode="nearest"), at integer ratios and at 88/26 x 112/62."""
import copy
import ctypes
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import downsize_oracle as O

pytestmark = pytest.mark.gpu

COST_SENTINEL, WS_TAIL, WS_TAIL_BYTES = -7.0, 0xA5, 4096
_ops, _chains, _modules = {}, {}, {}


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


def _f32(t):
    """a float64 tensor of fp32 values -> fp32 on the device, nothing lost"""
    f = t.float()
    assert torch.equal(f.double(), t)
    return f.to(_dev()).contiguous()


def _forward(image, start, goal, plus, depth, wts, scale, shift, mul):
    """One call of nastar_encoder_cnn_downsize_forward on fp32 device tensors (image [B,C,H,W], start / goal [B,h,w] or None, wts / scale /
    shift lists of depth + 1 tensors) -> (cost [B,Ho,Wo], [prep tensor, pooled levels]), copies taken after the sentinel checks."""
    from neural_astar import _native
    lib = _native.load()
    dev = _dev()
    B, C, H, W = image.shape
    Cin = C + int(plus)
    h, w = (start.shape[-2], start.shape[-1]) if plus else (0, 0)
    for t in [image] + ([start, goal] if plus else []) + list(wts) + list(scale) + list(shift):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
    cin_p = O.cin_pad(Cin)
    for l in range(depth + 1):  # the buffers the kernels index without a bound of their own
        cout_p = O.HIDDEN[l] if l < depth else O.FINAL_COUTP
        assert wts[l].shape == (9, cin_p, cout_p) and scale[l].shape == shift[l].shape == (cout_p,)
        cin_p = cout_p
    lv, ws_bytes = O.levels(B, Cin, H, W, depth)
    assert int(lib.nastar_encoder_downsize_workspace_bytes(B, Cin, H, W, depth)) == ws_bytes
    ws = torch.empty((ws_bytes + WS_TAIL_BYTES,), dtype=torch.uint8, device=dev)
    ws[:ws_bytes] = 0xFF
    ws[ws_bytes:] = WS_TAIL
    Ho, Wo = H >> depth, W >> depth
    cost = torch.full((B + 1, Ho, Wo), COST_SENTINEL, dtype=torch.float32, device=dev)
    arr = ctypes.c_void_p * (depth + 1)
    ptrs = lambda ts: arr(*[t.data_ptr() for t in ts])
    with torch.cuda.device(dev):
        rc = lib.nastar_encoder_cnn_downsize_forward(
            image.data_ptr(), start.data_ptr() if plus else None, goal.data_ptr() if plus else None, int(plus), B, C, H, W, h, w, depth,
            ptrs(wts), ptrs(scale), ptrs(shift), float(mul), cost.data_ptr(), ws.data_ptr(), ws_bytes, torch.cuda.current_stream(dev).cuda_stream)
    _native.check(rc, "nastar_encoder_cnn_downsize_forward")
    torch.cuda.synchronize()
    assert bool((ws[ws_bytes:] == WS_TAIL).all()), "the call wrote past workspace_bytes"
    assert bool((cost[B] == COST_SENTINEL).all()), "the call wrote past image B - 1 of cost_out"
    body = ws[:ws_bytes].view(torch.float32)
    got = [body[off:off + math.prod(shp)].view(shp).clone() for off, shp in lv]
    out = cost[:B].clone()
    for l, t in enumerate(got + [out]):
        assert not bool(torch.isnan(t).any()), "level %d holds a NaN: an element the launch did not write, or made from one" % l
    return out, got


def _exact(case, hw=None):
    """exact operands of a case (float64, CPU) with their fp32 device copies, and the oracle's chain: computed once"""
    return _prepared((case, hw), lambda: O.exact_operands(*case, hw=hw))


def _prepared(key, make):
    if key not in _ops:
        ops = make()
        ops["dev"] = dict(image=_f32(ops["image"]), start=_f32(ops["start"]) if ops["plus"] else None,
                          goal=_f32(ops["goal"]) if ops["plus"] else None,
                          wts=[_f32(t) for t in ops["wts"]], scale=[_f32(t) for t in ops["scale"]], shift=[_f32(t) for t in ops["shift"]])
        _ops[key] = ops
        lv, z, _ = O.chain(ops["image"], ops["start"], ops["goal"], ops["plus"], ops["wts"], ops["scale"], ops["shift"], 1.0)
        _chains[key] = (lv, z)
    return _ops[key], _chains[key]


def _run_exact(ops, mul, b0=0, B=None, **replace):
    d = dict(ops["dev"], **replace)
    B = ops["B"] if B is None else B
    cut = lambda t: t[b0:b0 + B].contiguous() if t is not None else None
    return _forward(cut(d["image"]), cut(d["start"]), cut(d["goal"]), ops["plus"], ops["depth"], d["wts"], d["scale"], d["shift"], mul)


def _check_exact(ops, chain, mul, what):
    """precondition, launch, every level equal to the oracle's bits, the cost map within the suite's bound of the float64 sigmoid"""
    lv, z = chain
    assert max(O.exactness(ops)) < O.EXACT_LIMIT, "operands that can round in fp32 prove nothing here"
    cost, got = _run_exact(ops, mul)
    assert len(got) == len(lv) == ops["depth"] + 1
    for l, (g, want) in enumerate(zip(got, lv)):
        want32 = want.float()
        assert torch.equal(want32.double(), want)
        g = g.cpu()
        assert g.shape == want32.shape
        bad = (g != want32)
        assert torch.equal(g, want32), "%s: level %d (0 = prep tensor) differs at %d of %d elements, first at [b,y,x,c] = %s" % (
            what, l, int(bad.sum()), bad.numel(), bad.nonzero()[0].tolist())
    truth = mul * torch.sigmoid(z)
    assert cost.shape == truth.shape
    err = float((cost.cpu().double() - truth).abs().max())
    print(f"{what} final_mul={mul}: max |cost - float64 sigmoid| = {err:.3e} (pre-activation in [{float(z.min()):.3f}, {float(z.max()):.3f}])")
    assert err <= 1e-5 * max(1.0, mul), err
    return cost, got


# ---- A: bit-exact levels -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mul", O.FINAL_MULS)
@pytest.mark.parametrize("case", O.CASES, ids=O.case_id)
def test_every_level_has_the_oracles_bits(case, mul):
    ops, chain = _exact(case)
    cost, got = _check_exact(ops, chain, mul, O.case_id(case))
    # the last block's 31 padded channels carry weights, scales and shifts here; with all of them zero the cost map keeps its bits
    d, last = ops["dev"], ops["depth"]
    assert bool(d["wts"][last][:, :, 1:].any()) and bool(d["scale"][last][1:].all())
    zeroed = {}
    for name in ("wts", "scale", "shift"):
        t = d[name][last].clone()
        t[..., 1:] = 0
        zeroed[name] = d[name][:last] + [t]
    cost0, _ = _run_exact(ops, mul, **zeroed)
    assert torch.equal(cost0, cost), "a padded output channel of the last block reached cost_out"


# ---- B: batch independence ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in O.CASES if c[2:4] in ((24, 40), (16, 16))], ids=O.case_id)
def test_an_image_alone_has_its_bits_in_the_batch(case):
    ops, _ = _exact(case)
    B = ops["B"]
    cost, got = _run_exact(ops, 10.0)
    for b in sorted({0, B // 2, B - 1}):
        cost1, got1 = _run_exact(ops, 10.0, b0=b, B=1)
        assert torch.equal(cost1[0], cost[b]), "cost map of image %d" % b
        for l, (one, many) in enumerate(zip(got1, got)):
            assert torch.equal(one[0], many[b]), "level %d of image %d" % (l, b)


# ---- C: ordinary numbers through the wrapper ------------------------------------------------------------------------------------------------
def _module(kind, depth, const):
    """a random CNNDownSize with non-trivial BatchNorm statistics and affine parameters, in eval mode on the device"""
    key = (kind, depth, const)
    if key not in _modules:
        from neural_astar.planner.encoder import CNNDownSize
        C, plus = O.KINDS[kind]
        torch.manual_seed(7 + 13 * depth + len(kind))
        cnn = CNNDownSize(C + plus, depth, const)
        with torch.no_grad():
            for m in cnn.model:
                if isinstance(m, nn.BatchNorm2d):
                    m.running_mean.normal_(0, 0.3); m.running_var.uniform_(0.5, 1.5)
                    m.weight.uniform_(0.5, 1.5); m.bias.normal_(0, 0.2)
        _modules[key] = cnn.to(_dev()).eval()
    return _modules[key]


def _truth(cnn, images, start, goal, plus):
    """the torch module in float64 on the CPU: images [B,C,H,W], start / goal [B,1,h,w] -> [B,1,Ho,Wo] float64"""
    c64 = copy.deepcopy(cnn).cpu().double().eval()
    x = O.prep(images.cpu(), start.cpu()[:, 0], goal.cpu()[:, 0], plus, images.shape[1] + int(plus)).permute(0, 3, 1, 2)
    with torch.no_grad():
        return c64(x)


def _problem(kind, depth, H, W, B, seed):
    C, plus = O.KINDS[kind]
    g = torch.Generator().manual_seed(seed)
    images = torch.rand((B, C, H, W), generator=g).to(_dev())
    h, w = H >> depth, W >> depth
    start, goal = (O.one_hot(B, h, w, g).float().unsqueeze(1).to(_dev()) for _ in range(2))
    return images, start, goal, plus


def _bound(cnn):
    const = cnn.const
    return 1e-5 * max(1.0, float(const.detach().item()) if isinstance(const, torch.Tensor) else float(const))


@pytest.mark.parametrize("const", [None, 10.0])
@pytest.mark.parametrize("case", O.CASES, ids=O.case_id)
def test_wrapper_matches_the_float64_module(case, const):
    from neural_astar.encoder_hip import HipCnnDownSizeEncoder
    kind, depth, H, W, B = case
    cnn = _module(kind, depth, const)
    enc = HipCnnDownSizeEncoder(cnn)
    images, start, goal, plus = _problem(kind, depth, H, W, B, seed=H + W)
    got = enc(images, start, goal, plus)
    want = _truth(cnn, images, start, goal, plus)
    assert got.shape == want.shape == (B, 1, H >> depth, W >> depth)
    if want.numel() > 8:
        assert float(want.std()) > 1e-3, "degenerate cost map: the test would not see the layers"
    err = float((got.cpu().double() - want).abs().max())
    print(f"{O.case_id(case)} const={const}: max |wrapper - float64 module| = {err:.3e}")
    assert err <= _bound(cnn), err


# ---- D: the wrapper's caches ----------------------------------------------------------------------------------------------------------------
D_CASE = ("rgb+", 3, 24, 40)


@pytest.fixture(scope="module")
def cached_encoder():
    """one encoder object for all of D, on a module of its own (the tests change its parameters)"""
    from neural_astar.encoder_hip import HipCnnDownSizeEncoder
    cnn = copy.deepcopy(_module(D_CASE[0], D_CASE[1], 10.0))
    return HipCnnDownSizeEncoder(cnn)


def test_wrapper_follows_every_change_of_the_module(cached_encoder):
    enc, cnn = cached_encoder, cached_encoder.cnn
    kind, depth, H, W = D_CASE
    images, start, goal, plus = _problem(kind, depth, H, W, 3, seed=3)
    g = torch.Generator().manual_seed(99)
    bns = [m for m in cnn.model if isinstance(m, nn.BatchNorm2d)]

    def in_place_update():
        for p in cnn.model.parameters():
            p.add_(0.2 * p.abs().mean() * torch.randn(p.shape, generator=g).to(p.device))

    def running_statistics():
        for m in bns:
            m.running_mean.add_(0.25)
            m.running_var.mul_(1.6)

    def load_state_dict():
        from neural_astar.planner.encoder import CNNDownSize
        torch.manual_seed(1234)
        other = CNNDownSize(4, depth, 10.0)
        for m in other.model:
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.3); m.running_var.uniform_(0.5, 1.5)
        cnn.load_state_dict(other.state_dict())

    def const_in_place():
        cnn.const.fill_(4.0)

    seen = [enc(images, start, goal, plus).cpu().double()]
    err = float((seen[0] - _truth(cnn, images, start, goal, plus)).abs().max())
    assert err <= _bound(cnn), ("first call", err)
    for change in (in_place_update, running_statistics, load_state_dict, const_in_place):
        with torch.no_grad():
            change()
        want = _truth(cnn, images, start, goal, plus)
        moved = float((want - seen[-1]).abs().max())
        assert moved > 100 * _bound(cnn), "%s moved the truth by %.1e only: a stale cache would pass" % (change.__name__, moved)
        got = enc(images, start, goal, plus).cpu().double()
        err = float((got - want).abs().max())
        print(f"after {change.__name__}: truth moved by {moved:.3e}, max |wrapper - float64 module| = {err:.3e}")
        assert err <= _bound(cnn), (change.__name__, err)
        seen.append(got)


def test_wrapper_follows_a_plain_float_const():
    """const=None leaves the module's const the float 1.0 (reference encoder.py:27), which is no parameter and has no version"""
    from neural_astar.encoder_hip import HipCnnDownSizeEncoder
    kind, depth, H, W = D_CASE
    cnn = copy.deepcopy(_module(kind, depth, None))
    enc = HipCnnDownSizeEncoder(cnn)
    images, start, goal, plus = _problem(kind, depth, H, W, 2, seed=4)
    first = enc(images, start, goal, plus).cpu().double()
    assert float((first - _truth(cnn, images, start, goal, plus)).abs().max()) <= _bound(cnn)
    cnn.const = 6.0
    got = enc(images, start, goal, plus).cpu().double()
    want = _truth(cnn, images, start, goal, plus)
    assert float((want - first).abs().max()) > 100 * _bound(cnn)
    assert float((got - want).abs().max()) <= _bound(cnn)


def test_wrapper_keeps_its_bits_on_a_cached_larger_workspace(cached_encoder):
    enc = cached_encoder
    kind, depth, H, W = D_CASE
    images, start, goal, plus = _problem(kind, depth, H, W, 9, seed=5)
    first = enc(images[:2], start[:2], goal[:2], plus).clone()
    nine = enc(images, start, goal, plus).clone()
    ws = enc._ws
    again = enc(images[:2], start[:2], goal[:2], plus)
    assert enc._ws is ws, "the larger workspace was not kept"
    assert torch.equal(again, first)
    assert torch.equal(nine[:2], first)


def test_wrapper_takes_views_that_are_not_contiguous(cached_encoder):
    enc = cached_encoder
    kind, depth, H, W = D_CASE
    images, start, goal, plus = _problem(kind, depth, H, W, 3, seed=6)
    want = enc(images, start, goal, plus).clone()
    wide = torch.rand((3, 5, H, W), device=_dev())
    wide[:, 1:4] = images
    sg = torch.cat((start, goal), dim=1)
    img_v, s_v, g_v = wide[:, 1:4], sg[:, 0:1], sg[:, 1:2]
    assert not img_v.is_contiguous() and not s_v[:, 0].is_contiguous() and not g_v[:, 0].is_contiguous()
    got = enc(img_v, s_v, g_v, plus)
    assert torch.equal(got, want)


def test_wrapper_refuses_training_mode(cached_encoder):
    enc = cached_encoder
    kind, depth, H, W = D_CASE
    images, start, goal, plus = _problem(kind, depth, H, W, 2, seed=7)
    enc.cnn.train()
    try:
        with pytest.raises(RuntimeError):
            enc(images, start, goal, plus)
    finally:
        enc.cnn.eval()


# ---- E: start + goal upsampling ---------------------------------------------------------------------------------------------------------------
def _upsampled(start, goal, H, W):
    """the reference's own operation on fp32 tensors, on the CPU: [B,h,w] -> [B,H,W]"""
    return F.interpolate((start.float() + goal.float()).unsqueeze(1), size=(H, W), mode="nearest")[:, 0]


@pytest.mark.parametrize("full", [False, True], ids=["pooled-size", "full-size"])
@pytest.mark.parametrize("case", O.UPSAMPLE_CASES, ids=O.case_id)
def test_start_goal_channel_at_integer_ratios(case, full):
    kind, depth, H, W, B = case
    hw = O.upsample_sizes(case)[int(full)]
    assert hw == ((H, W) if full else (H >> depth, W >> depth))
    ops, chain = _exact(case, hw=hw)
    assert ops["start"].shape == (B,) + hw
    _, got = _check_exact(ops, chain, 1.0, O.case_id(case) + " start/goal %dx%d" % hw)
    want = _upsampled(ops["start"], ops["goal"], H, W)
    assert float(want.sum()) >= B
    assert torch.equal(got[0][..., ops["C"]].cpu(), want)


@pytest.mark.parametrize("pattern", O.NONINTEGER_PATTERNS)
def test_start_goal_channel_at_a_ratio_that_is_no_integer(pattern):
    """88 x 112 from 26 x 62: at output row 44 and output column 56 F.interpolate shows another source row and column than
    (y * h) // H does.  The oracle names them; the one-hot maps sit on both candidates, the dense map covers every cell."""
    H, W, h, w = O.NONINTEGER_RATIO
    ops, (lv, z) = _prepared(("noninteger", pattern), lambda: O.noninteger_operands(pattern))
    start, goal = ops["start"], ops["goal"]
    want = _upsampled(start, goal, H, W)
    by_integers = (start + goal)[0][O.integer_source_index(h, H)][:, O.integer_source_index(w, W)].float()
    assert not torch.equal(by_integers, want[0]), "the case would not tell the two formulas apart"
    assert torch.equal(lv[0][0, :, :, 1].float(), want[0])
    _, got = _check_exact(ops, (lv, z), 1.0, "m+ 88x112 from 26x62 " + pattern)
    assert torch.equal(got[0][0, :, :, 1].cpu(), want[0])
