"""The eval-mode CNN encoder (csrc/nastar_encoder.hip.h, launch logic csrc/nastar_encoder_capi.hip) at its batch, chunk and CU-count
edges, through the three C entry points nastar_encoder_cnn_forward{,_f16,_f16x3} and the stand-alone layer nastar_conv3x3_img32_f16.

The invariant is BIT IDENTITY.  For a precision and a map size the kernel route depends on H, W and NASTAR_ENCODER_FLAGS only -- not on
B, not on the images per pass, not on the workgroup an item lands on -- and every work item runs the same instruction sequence on the
same operands.  The cost map of image b therefore has the same bits in a batch of 2 or 3 as in one of CU count + 3, in one pass as in
three, first as last.  Every comparison below is torch.equal; no tolerance stands in for it.

Accuracy is anchored once per route on a small batch against the torch module evaluated in float64 on the CPU, with the bounds the
suite already uses for these encoders (bf16: max < 3e-2, mean < 3e-3; f16: max < 5e-3, mean < 5e-4; f16x3: max < 1e-5 * max(1,
const)); bit identity carries that accuracy to every image of every other run.

A  the chunk loop (`chunk = workspace_bytes / per_image`, slabs laid out from `chunk`, inputs and cost_out advanced per pass, a short
   last pass) against a single pass with the workspace the library asks for;
B  the persistent workgroups: whole encoder at B = 5 (grids below 8: no XCD permutation), 8 (grids 8 and 16: permuted),
   n_cu + 3 (three workgroups take a second image in the stem and the fused last layer, the middle layer has 2 n_cu + 6 items) on 32x32
   maps; B = 3 and 45 on 64x96 maps (2 x 3 tiles per image: a workgroup walks from an interior-edge tile to a corner tile, where a stale
   halo ring would show); the tiled (NASTAR_ENCODER_FLAGS=1) and separate-last-layer (8) routes of the bf16 form;
C  the same persistent kernel as the stand-alone fp16 layer of the training forward and the input gradient, all five (cin, cout)
   pairs, plain and split, at more work items than CUs with a remainder.

Expected rows of a large batch come from runs of 2 (64x96) or 3 (32x32) or 4 (C) images through the same helper: one item per
workgroup at most, no permutation.  Every call gets a cost_out one image longer than B and a workspace 4 KiB longer than the
workspace_bytes it is told, both pre-filled with a sentinel that must survive, so a tail pass that overruns either is seen."""
import copy
import ctypes
import os

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

PRECISIONS = ("bf16", "f16", "f16x3")
CONST = 3.0
BOUNDS = {"bf16": (3e-2, 3e-3), "f16": (5e-3, 5e-4), "f16x3": (1e-5 * max(1.0, CONST), None)}  # (max, mean) against float64
WS_SENTINEL, COST_SENTINEL = 0xA5, -7.0

_planners, _encoders, _pools, _truths, _rows = {}, {}, {}, {}, {}


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


def _n_cu():
    return int(torch.cuda.get_device_properties(_dev()).multi_processor_count)


def _planner(enc_in):
    """NeuralAstar with the depth-4 CNN, const = 3 and non-trivial BatchNorm statistics / affine parameters (eval mode), on the device"""
    if enc_in not in _planners:
        from neural_astar.planner import NeuralAstar
        torch.manual_seed(5 + len(enc_in))
        na = NeuralAstar(encoder_input=enc_in, encoder_arch="CNN", const=CONST).to(_dev())
        with torch.no_grad():
            for mod in na.encoder.model:
                if isinstance(mod, nn.BatchNorm2d):
                    mod.running_mean.normal_(0, 0.2); mod.running_var.uniform_(0.5, 1.5)
                    mod.weight.uniform_(0.5, 1.5); mod.bias.normal_(0, 0.2)
        _planners[enc_in] = na.eval()
    return _planners[enc_in]


def _encoder(precision, enc_in="m+"):
    if (precision, enc_in) not in _encoders:
        from neural_astar.encoder_hip import HipCnnEncoder
        _encoders[(precision, enc_in)] = HipCnnEncoder(_planner(enc_in).encoder, precision)
    return _encoders[(precision, enc_in)]


def _pool(H, W, n=0):
    """Distinct problems of H x W (random obstacle maps, one-hot start and goal) as [N,H,W] fp32 device tensors, N = the largest batch
    any test here uses at this size; image b of every batch is image b of the pool"""
    if (H, W) not in _pools:
        from neural_astar.utils import synthetic as syn
        N = {(32, 32): _n_cu() + 3, (64, 96): _batch("tiles>cu", _n_cu())}.get((H, W), 8)
        pr = syn.random_obstacle_maps(N, H, W, 0.2, seed=17 + H + W)
        _pools[(H, W)] = tuple(torch.from_numpy(x[:, 0]).to(_dev()).contiguous() for x in pr)
    assert _pools[(H, W)][0].shape[0] >= n
    return _pools[(H, W)]


def _truth(H, W, enc_in, n):
    """the torch module in float64 on the CPU for the first n images of the pool: [n,H,W] fp32"""
    have = _truths.get((H, W, enc_in))
    if have is None or have.shape[0] < n:
        m, s, g = (t[:n].cpu().double().unsqueeze(1) for t in _pool(H, W, n))
        cnn = copy.deepcopy(_planner(enc_in).encoder).cpu().double().eval()
        with torch.no_grad():
            have = _truths[(H, W, enc_in)] = cnn(torch.cat((m, s + g), dim=1) if enc_in == "m+" else m)[:, 0].float()
    return have[:n]


def _entry(lib, precision):
    return {"bf16": (lib.nastar_encoder_cnn_forward, lib.nastar_encoder_workspace_bytes),
            "f16": (lib.nastar_encoder_cnn_forward_f16, lib.nastar_encoder_workspace_bytes_f16),
            "f16x3": (lib.nastar_encoder_cnn_forward_f16x3, lib.nastar_encoder_workspace_bytes_f16x3)}[precision]


def _forward(precision, H, W, b0, B, enc_in="m+", ws_images=None, ws_bytes=None):
    """Images b0 .. b0 + B - 1 of the pool through the C entry point of `precision` with a workspace of `ws_images` images (or of
    `ws_bytes` bytes; default: what the library asks for B images = one pass).  Returns the cost maps [B,H,W] (a copy)."""
    from neural_astar import _native
    lib = _native.load()
    dev = _dev()
    enc = _encoder(precision, enc_in)
    fwd, ws_fn = _entry(lib, precision)
    per_image = int(ws_fn(1, H, W))
    assert per_image > 0
    if ws_bytes is None:
        ws_bytes = int(ws_fn(B, H, W)) if ws_images is None else ws_images * per_image
    m, s, g = (t[b0:b0 + B] for t in _pool(H, W, b0 + B))
    assert m.is_contiguous() and m.shape == (B, H, W)
    plus = enc_in == "m+"
    cost = torch.full((B + 1, H, W), COST_SENTINEL, dtype=torch.float32, device=dev)
    ws = torch.full((ws_bytes + 4096,), WS_SENTINEL, dtype=torch.uint8, device=dev)
    arr = ctypes.c_void_p * 5
    ptrs = lambda ts: arr(*[t.data_ptr() for t in ts])
    head = (m.data_ptr(), s.data_ptr() if plus else None, g.data_ptr() if plus else None, int(plus), B, H, W)
    tail = (ptrs(enc.scale), ptrs(enc.shift), enc._mul, cost.data_ptr(), ws.data_ptr(), ws_bytes, torch.cuda.current_stream(dev).cuda_stream)
    with torch.cuda.device(dev):
        if precision == "bf16":
            rc = fwd(*head, ptrs(enc.wpack), *tail)
        else:
            rc = fwd(*head, enc.w1.data_ptr(), ptrs(enc.wsplit), *tail)
    _native.check(rc, "nastar_encoder_cnn_forward[%s]" % precision)
    torch.cuda.synchronize()
    assert bool((ws[ws_bytes:] == WS_SENTINEL).all()), "the call wrote past workspace_bytes"
    assert bool((cost[B] == COST_SENTINEL).all()), "the call wrote past image B - 1 of cost_out"
    out = cost[:B].clone()
    assert bool(((out >= 0) & (out <= CONST)).all()), "a cost map was not written (or is outside [0, const])"
    return out


def _expected_rows(precision, H, W, B, enc_in="m+", flags=""):
    """rows 0 .. B - 1 from runs of 3 (32x32) or 2 (other sizes) images each, one pass per run; computed once per route and kept"""
    key = (precision, H, W, enc_in, flags)
    have = _rows.get(key)
    if have is None or have.shape[0] < B:
        step = 3 if (H, W) == (32, 32) else 2
        _pool(H, W, B)
        have = _rows[key] = torch.cat([_forward(precision, H, W, b0, min(step, B - b0), enc_in) for b0 in range(0, B, step)])
    return have[:B]


def _anchor(got, precision, H, W, enc_in, what):
    """`got` = rows 0 .. n - 1 of a route against the float64 torch module, within the suite's bounds for `precision`"""
    truth = _truth(H, W, enc_in, got.shape[0])
    assert float(truth.std()) > 1e-3, "degenerate cost map: the test would not see the layers"
    err = (got.cpu() - truth).abs()
    emax, emean = float(err.max()), float(err.mean())
    print(f"anchor {what}: {precision} {H}x{W} {enc_in} n={got.shape[0]}: max |hip - float64| = {emax:.3e}, mean = {emean:.3e}")
    bmax, bmean = BOUNDS[precision]
    assert emax < bmax, (what, emax)
    if bmean is not None:
        assert emean < bmean, (what, emean)


def _first_difference(got, want):
    bad = (got != want).flatten(1).any(1).nonzero().flatten().tolist()
    return "images that differ: %s of %d" % (bad[:16], got.shape[0])


# ---- A: the chunk loop ------------------------------------------------------------------------------------------------------------------
CHUNK_CASES = [  # H, W, encoder input, B, images the workspace holds
    (32, 32, "m+", 8, 3),   # passes of 3, 3, 2: stem + img32<64,128> + fused last layer (f16x3: first_f32 + two img32 + fused)
    (32, 32, "m", 5, 2),    # passes of 2, 2, 1; plus = 0 with NULL start and goal
    (64, 96, "m+", 5, 2),   # the 32x32-tile route + the stand-alone last layer (f16x3: three accumulating passes through zacc)
    (16, 32, "m+", 5, 2),   # bf16 only: the generic tiled kernel (the fp16 forms refuse H % 32 != 0)
]


@pytest.mark.parametrize("H,W,enc_in,B,holds,precision",
                         [c + (p,) for c in CHUNK_CASES for p in PRECISIONS if c[0] % 32 == 0 or p == "bf16"], ids=lambda v: str(v))
def test_chunked_passes_equal_a_single_pass(H, W, enc_in, B, holds, precision):
    _pool(H, W, B)
    single = _forward(precision, H, W, 0, B, enc_in)
    _anchor(single, precision, H, W, enc_in, "single pass")
    chunked = _forward(precision, H, W, 0, B, enc_in, ws_images=holds)
    assert torch.equal(chunked, single), _first_difference(chunked, single)
    one = _forward(precision, H, W, 0, B, enc_in, ws_images=1)  # B passes of one image: every offset, every slab at its smallest
    assert torch.equal(one, single), _first_difference(one, single)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_workspace_one_byte_short_of_four_images_is_one_of_three(precision):
    """64x96, B = 5: 4 * per_image - 1 bytes hold 3 images (passes of 3 and 2).  Slabs laid out for 4 would end one byte past the
    workspace: the widest bf16 slab and the f16x3 partial-sum slab are written to their last byte on this route, into the sentinel."""
    from neural_astar import _native
    H, W, B = 64, 96, 5
    per_image = int(_entry(_native.load(), precision)[1](1, H, W))
    _pool(H, W, B)
    single = _forward(precision, H, W, 0, B)
    short = _forward(precision, H, W, 0, B, ws_bytes=4 * per_image - 1)
    assert torch.equal(short, single), _first_difference(short, single)
    three = _forward(precision, H, W, 0, B, ws_images=3)
    assert torch.equal(three, single), _first_difference(three, single)


# ---- B: persistent scheduling, whole encoder --------------------------------------------------------------------------------------------
def _batch(spec, n_cu):
    if spec == "cu+3":
        return n_cu + 3
    if spec == "tiles>cu":  # 64x96: 6 tiles per image; 45 images = 270 / 540 / 1080 items at 256 CUs, more on a larger device
        B = max(45, n_cu // 6 + 3)
        assert B * 6 > n_cu
        return B
    return int(spec)


def _grids(precision, H, W, B, n_cu, flags=0):
    """launch grids of the persistent kernels on this route (csrc/nastar_encoder_capi.hip), for the log"""
    tiles = (H // 32) * (W // 32)
    cap = lambda items: min(items, n_cu)
    if (H, W) == (32, 32):
        if flags & 1:
            return "generic tiled kernels only (not persistent)"
        mid = "img32<64,128> %d" % cap(2 * B)
        if precision == "f16x3":
            return "first_f32, img32<32,64> %d, %s, fused %d" % (cap(B), mid, cap(B))
        last = "img32<128,256> %d + final" % cap(4 * B) if flags & 8 else "fused %d" % cap(B)
        return "stem %d, %s, %s" % (cap(B), mid, last)
    return "tiled img32 %d, %d, %d (+ first layer, last layer: not persistent)" % (cap(B * tiles), cap(2 * B * tiles), cap(4 * B * tiles))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("H,W,spec", [(32, 32, "5"), (32, 32, "8"), (32, 32, "cu+3"), (64, 96, "3"), (64, 96, "tiles>cu")])
def test_every_image_of_a_batch_has_the_bits_of_its_small_run(H, W, spec, precision):
    n_cu = _n_cu()
    B = _batch(spec, n_cu)
    print(f"{precision} {H}x{W} B={B} n_cu={n_cu}: {_grids(precision, H, W, B, n_cu)}")
    _pool(H, W, B)
    want = _expected_rows(precision, H, W, B)
    _anchor(want[:6], precision, H, W, "m+", "small runs")
    got = _forward(precision, H, W, 0, B)
    assert torch.equal(got, want), _first_difference(got, want)


@pytest.mark.parametrize("flags", ["1", "8"])
def test_bf16_tiled_and_separate_last_layer_routes_at_more_images_than_cus(flags):
    """NASTAR_ENCODER_FLAGS = 1 (generic tiled kernels for 32x32 maps) and 8 (the last layer a launch of its own: img32<128,256> walks
    4 B items) at B = n_cu + 3, each against its own small runs under the same flag"""
    n_cu = _n_cu()
    B = n_cu + 3
    print(f"bf16 32x32 B={B} n_cu={n_cu} flags={flags}: {_grids('bf16', 32, 32, B, n_cu, int(flags))}")
    _pool(32, 32, B)
    try:
        os.environ["NASTAR_ENCODER_FLAGS"] = flags
        want = _expected_rows("bf16", 32, 32, B, flags=flags)
        got = _forward("bf16", 32, 32, 0, B)
    finally:
        os.environ.pop("NASTAR_ENCODER_FLAGS", None)
    _anchor(want[:6], "bf16", 32, 32, "m+", "small runs, flags " + flags)
    assert torch.equal(got, want), _first_difference(got, want)
    plain = _expected_rows("bf16", 32, 32, 6)
    assert not torch.equal(plain, want[:6]), "the flag did not change the route (same bits as the default route)"


# ---- C: the persistent kernel as a stand-alone layer ------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("cin,cout", [(32, 64), (64, 128), (128, 256), (256, 128), (128, 64)])
def test_img32_layer_rows_at_more_items_than_cus(cin, cout, split):
    """nastar_conv3x3_img32_f16 with ReLU: B * cout / 64 work items exceed n_cu with a remainder; every image has the bits of its run of 4"""
    from neural_astar import _native, encoder_hip as E
    lib = _native.load()
    dev = _dev()
    n_cu = _n_cu()
    B = {64: n_cu + 3, 128: n_cu // 2 + 3, 256: n_cu // 4 + 6}[cout]
    items = B * (cout // 64)
    assert items > n_cu and items % n_cu != 0
    print(f"img32 layer {cin}->{cout} split={int(split)} B={B}: {items} items on {n_cu} workgroups")
    g = torch.Generator().manual_seed(cin * 3 + cout + int(split))
    conv = nn.Conv2d(cin, cout, 3, padding=1)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (2.0 / (9 * cin)) ** 0.5)
        conv.bias.copy_(torch.randn(cout, generator=g))
    wpack, scale, shift, _, _ = E.pack_flat_conv(conv, None, split)
    wpack, scale, shift = wpack.to(dev), scale.to(dev), shift.to(dev)
    M = 2 if split else 1
    gd = torch.Generator(device=dev).manual_seed(cin + cout)
    x = torch.randn((B, 32, 32, cin), generator=gd, device=dev)
    hi = x.to(torch.float16)
    xin = (torch.cat((hi, (x - hi.float()).to(torch.float16)), dim=-1) if split else hi).contiguous()
    flags = E.CONV_RELU | (E.CONV_SPLIT if split else 0)
    st = torch.cuda.current_stream(dev).cuda_stream

    def run(b0, nb):
        out = torch.full((nb + 1, 32, 32, cout * M), 7.0, dtype=torch.float16, device=dev)
        _native.check(lib.nastar_conv3x3_img32_f16(xin[b0:].data_ptr(), wpack.data_ptr(), scale.data_ptr(), shift.data_ptr(), out.data_ptr(), nb,
                                                   cin, cout, flags, st), "nastar_conv3x3_img32_f16")
        torch.cuda.synchronize()
        assert bool((out[nb] == 7.0).all()), "the layer wrote past image B - 1"
        return out[:nb].view(torch.int16)

    want = torch.cat([run(b0, min(4, B - b0)) for b0 in range(0, B, 4)])
    got = run(0, B)
    assert torch.equal(got, want), _first_difference(got, want)
    v = got.view(torch.float16)
    assert bool(torch.isfinite(v).all()) and float(v[..., :cout].float().std()) > 1e-2, "degenerate layer output"
