"""The encoder's streaming training kernels (csrc/nastar_encoder_train.hip.h, csrc/nastar_encoder_co1.hip.h) called through the C ABI at
their edge shapes and held against the float64 definitions of tests/encoder_stream_oracle.py, each output within the bound derived there
(no tolerance constant: ``ratio <= 1``).  Output buffers and workspaces start as NaN, so an element no lane wrote fails its comparison.

Every comparison prints ``EDGE <entry point> <case> n=<roundings> ratio=<error / bound>``; with NASTAR_EDGE_RATIOS_OUT=<file> the largest
ratio per entry point and case is also written there as JSON (profiles/encoder_stream_edges.json is such a run).  Nothing here reads it.
"""
import json
import os

import pytest
import torch
import torch.nn.functional as F

import encoder_stream_oracle as O

pytestmark = pytest.mark.gpu

NAN = float("nan")
EPS, MOM = 1e-5, 0.1
RATIOS = {}


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


def _lib():
    from neural_astar import _native
    return _native.load(), _native


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


@pytest.fixture(scope="module", autouse=True)
def _ratio_record():
    yield
    path = os.environ.get("NASTAR_EDGE_RATIOS_OUT")
    if path and RATIOS:
        with open(path, "w") as f:
            json.dump(RATIOS, f, indent=1, sort_keys=True)


def _check(entry, case, got, ref, bound, n=None):
    r = O.ratio(got, ref, bound)
    slot = RATIOS.setdefault(entry, {}).setdefault(case, {"ratio": 0.0})
    slot["ratio"] = max(slot["ratio"], r)
    if n is not None:
        slot["n"] = n
    print(f"EDGE {entry} {case} n={n} ratio={r:.3g}")
    assert r <= 1.0, (entry, case, r)


def _exact(entry, case, ok):
    RATIOS.setdefault(entry, {}).setdefault(case, {"ratio": 0.0})
    assert ok, (entry, case)


def _nan(shape, dtype, dev):
    return torch.full(shape, NAN, dtype=dtype, device=dev)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _case_id(C, shape, split, extra=""):
    return "C%d_%dx%dx%d_%s%s" % (C, shape[0], shape[1], shape[2], "split" if split else "plain", extra)


# =================================================================================================================================
# the closing convolution as streams, and the BatchNorm-backward passes of the block in front of it that form its input gradient
# =================================================================================================================================
def _front_block(C, shape, split, seed):
    """a hidden block in front of the closing convolution: pre-activations z with no ambiguous ReLU decision under its own batch
    statistics, the block's coefficients, the closing weight, bias and the upstream gradient d"""
    B, H, W = shape
    g = torch.Generator().manual_seed(seed)
    z = torch.randn((B, C, H, W), generator=g) * 1.5 + 0.2
    gamma = torch.rand(C, generator=g) + 0.5
    beta = (torch.rand(C, generator=g) * 0.3 + 0.2) * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)  # away from 0: one pixel decides on beta
    w = torch.randn((1, C, 3, 3), generator=g) * 0.1
    bias = torch.randn(1, generator=g)
    d = torch.randn((B, H, W), generator=g)

    def coef(v):
        f = O.bn_forward(v, gamma, beta, EPS, MOM, None, None)
        return f["k2"].float().double(), f["k3"].float().double()

    z, zs = O.deambiguate(z, split, coef)
    fwd = O.bn_forward(zs, gamma, beta, EPS, MOM, None, None)
    k2f, k3f = fwd["k2"].float(), fwd["k3"].float()
    assert int(O.mask_ambiguous(zs, k2f.double(), k3f.double()).sum()) == 0
    return dict(z=z, zs=zs, gamma=gamma, beta=beta, w=w, bias=bias, d=d, fwd=fwd, k2f=k2f, k3f=k3f, g=g)


def _run_conv_family(C, shape, wgrad=True, splits=(False, True)):
    lib, N = _lib()
    dev = _dev()
    st = _stream(dev)
    B, H, W = shape
    npix = B * H * W
    for split in splits:
        blk = _front_block(C, shape, split, 1000 + C + 7 * npix)
        a_raw, a_seen = torch.relu(blk["z"]), torch.relu(blk["zs"])  # post-ReLU activations with their exact zeros (rounding to fp16 commutes with the ReLU)
        w_, bias_, d_ = blk["w"].to(dev), blk["bias"].to(dev), blk["d"].to(dev)
        k2_, k3_ = blk["k2f"].to(dev), blk["k3f"].to(dev)
        nb = int(lib.nastar_conv3x3_co1_workspace_bytes(B, H, W, C))
        assert nb >= npix * 9 * 4
        for fused in (False, True):
            src = blk["z"] if fused else a_raw
            a_ = O.nhwc(src, split).to(dev)
            av = blk["zs"] if fused else a_seen
            kk = (blk["k2f"].double(), blk["k3f"].double()) if fused else (None, None)
            case = _case_id(C, shape, split, "_fused" if fused else "")
            ws = _nan((nb // 4,), torch.float32, dev)
            z_out = _nan((B, H, W), torch.float32, dev)
            N.check(lib.nastar_conv3x3_co1_f16(a_.data_ptr(), w_.data_ptr(), bias_.data_ptr(), B, H, W, C, int(split), _ptr(k2_ if fused else None),
                                               _ptr(k3_ if fused else None), z_out.data_ptr(), ws.data_ptr(), nb, st), "co1")
            n = O.n_conv(C, fused)
            ref, bound = O.co1_forward(av, blk["w"], blk["bias"], n, *kk)
            _check("nastar_conv3x3_co1_f16", case, z_out, ref, bound, n)
            if not wgrad:
                continue
            ws = _nan((nb // 4,), torch.float32, dev)
            dw = _nan((1, C, 3, 3), torch.float32, dev)
            N.check(lib.nastar_conv3x3_co1_wgrad_f16(d_.data_ptr(), a_.data_ptr(), B, H, W, C, int(split), _ptr(k2_ if fused else None),
                                                     _ptr(k3_ if fused else None), dw.data_ptr(), ws.data_ptr(), nb, st), "co1 wgrad")
            n = O.n_wgrad(npix, C, fused)
            ref, bound = O.co1_wgrad(blk["d"], av, n, *kk)
            _check("nastar_conv3x3_co1_wgrad_f16", case, dw, ref, bound, n)


def _run_u1_family(C, shape, splits=(False, True)):
    lib, N = _lib()
    dev = _dev()
    st = _stream(dev)
    B, H, W = shape
    npix = B * H * W
    for split in splits:
        case = _case_id(C, shape, split)
        blk = _front_block(C, shape, split, 2000 + C + 7 * npix)
        zs, fwd, gamma = blk["zs"], blk["fwd"], blk["gamma"]
        S_in = 8.0
        u, e_u = O.co1_u1(blk["d"], blk["w"], S_in, (B, C, H, W))
        mask = ((O._cvec(blk["k2f"]) * zs + O._cvec(blk["k3f"])) > 0).double()
        dy, e_dy, S_dy = u * mask, e_u * mask, e_u * mask / (O.N_U1 * O.U24)
        bwd = O.bn_backward(zs, dy, gamma, fwd)
        bb = O.bn_backward_bounds(zs, dy, e_dy, gamma, fwd, bwd)
        z_, d_, w_ = O.nhwc(blk["z"], split).to(dev), blk["d"].to(dev), blk["w"].to(dev)
        ms_, mt_, gamma_ = blk["k2f"].to(dev), blk["k3f"].to(dev), gamma.to(dev)
        mean_, invstd_ = fwd["mean"].to(dev), fwd["invstd"].to(dev)
        gs_in = torch.full((1,), S_in, device=dev)
        nb = int(lib.nastar_chan_stats_workspace_bytes(npix, C))
        assert nb > 0
        # (1) statistics with the gradient formed on the fly
        ws = _nan((nb // 4,), torch.float32, dev)
        sums = _nan((C, 2), torch.float64, dev)
        amax = _nan((1,), torch.float32, dev)
        N.check(lib.nastar_chan_stats_u1_f16_ws(d_.data_ptr(), w_.data_ptr(), gs_in.data_ptr(), B, H, W, z_.data_ptr(), ms_.data_ptr(), mt_.data_ptr(),
                                                sums.data_ptr(), amax.data_ptr(), C, int(split), ws.data_ptr(), nb, st), "stats u1")
        _check("nastar_chan_stats_u1_f16_ws", case, sums[:, 0], bwd["sdy"], bb["sdy"], O.N_U1)
        _check("nastar_chan_stats_u1_f16_ws", case, sums[:, 1], bwd["sdyz"], bb["sdyz"], O.N_U1)
        amax_ref, e_amax = float(dy.abs().max()), float(e_dy.max())
        _check("nastar_chan_stats_u1_f16_ws", case, amax, torch.tensor([amax_ref]), torch.tensor([e_amax]), O.N_U1)
        # (2) statistics + coefficients
        ws = _nan((nb // 4,), torch.float32, dev)
        gs_out = _nan((1,), torch.float32, dev)
        dgamma, dbeta, c1, c2, c3 = (_nan((C,), torch.float32, dev) for _ in range(5))
        sums2 = _nan((C, 2), torch.float64, dev)
        N.check(lib.nastar_bn_stats_coef_bwd_u1_f16(d_.data_ptr(), w_.data_ptr(), B, H, W, z_.data_ptr(), ms_.data_ptr(), mt_.data_ptr(), C, int(split),
                                                    mean_.data_ptr(), invstd_.data_ptr(), gamma_.data_ptr(), gs_in.data_ptr(), gs_out.data_ptr(),
                                                    dgamma.data_ptr(), dbeta.data_ptr(), c1.data_ptr(), c2.data_ptr(), c3.data_ptr(), sums2.data_ptr(),
                                                    ws.data_ptr(), nb, st), "bn bwd u1")
        e = "nastar_bn_stats_coef_bwd_u1_f16"
        _exact(e, case, torch.equal(sums2, sums) and float(gs_in) == S_in)  # the same partial rows in the same order
        r = float(gs_out) / S_in
        kmax = float((gamma.double() * fwd["invstd"]).abs().max())
        assert O.scale_window_ok(r, 2.0 * kmax * amax_ref, -40, 40, amax_rel=e_amax / amax_ref if amax_ref > 0 else 0.0), (case, r, kmax, amax_ref)
        _check(e, case, dgamma.double().cpu() * S_in, bwd["dgamma"], bb["dgamma"], O.N_U1)
        _check(e, case, dbeta.double().cpu() * S_in, bwd["dbeta"], bb["dbeta"], O.N_U1)
        for name, t in (("c1", c1), ("c2", c2), ("c3", c3)):
            _check(e, case, t.double().cpu() / r, bwd[name], bb[name], O.N_U1)
        # (3) dz = c1 dy + c2 z + c3 with the gradient formed on the fly: against the kernel's own coefficients, then against the oracle's dz
        out = _nan(tuple(z_.shape), torch.float16, dev)
        N.check(lib.nastar_chan_affine_u1_f16(d_.data_ptr(), w_.data_ptr(), gs_in.data_ptr(), B, H, W, z_.data_ptr(), c1.data_ptr(), c2.data_ptr(),
                                              c3.data_ptr(), ms_.data_ptr(), mt_.data_ptr(), out.data_ptr(), C, int(split), st), "affine u1")
        got = O.from_nhwc(out, C, split)
        k = [t.double().cpu() for t in (c1, c2, c3)]
        ref = O._cvec(k[0]) * dy + O._cvec(k[1]) * zs + O._cvec(k[2])
        _check("nastar_chan_affine_u1_f16", case, got, ref, O.affine_bound(k[0], S_dy, k[1], zs, k[2], split, n_u=O.N_U1, u=dy), O.N_U1 + O.N_AFFINE)
        rc = [r * bwd[x] for x in ("c1", "c2", "c3")]
        bound = O.affine_bound(rc[0], S_dy, rc[1], zs, rc[2], split, n_u=O.N_U1, coef_bounds=[r * bb[x] for x in ("c1", "c2", "c3")], u=dy)
        _check("nastar_chan_affine_u1_f16", case + "_dz", got, r * bwd["dz"], bound, O.N_U1 + O.N_AFFINE)


@pytest.mark.parametrize("shape", O.CO1_SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("C", O.CO1_CHANNELS)
def test_closing_convolution_streams_at_edge_shapes(C, shape):
    _run_conv_family(C, shape)


SPLITS = pytest.mark.parametrize("split", [False, True], ids=["plain", "split"])


@SPLITS
def test_closing_convolution_streams_past_the_projection_and_weight_gradient_caps(split):
    _run_conv_family(*O.CO1_PAST_PROJ_CAP, splits=(split,))


@SPLITS
def test_closing_convolution_past_the_shift_pass_cap(split):
    """1052672 pixels: only the forward's shifted sum has a cap up there.  (The streamed weight gradient of a million pixels passes through
    5 + 256 + 1 fp32 roundings: its honest bound is wider than one pixel's term, so that shape could not tell a dropped pixel anyway.)"""
    _run_conv_family(*O.CO1_PAST_SHIFT_CAP, wgrad=False, splits=(split,))


@pytest.mark.parametrize("shape", O.CO1_SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("C", O.U1_CHANNELS)
def test_on_the_fly_gradient_passes_at_edge_shapes(C, shape):
    _run_u1_family(C, shape)


@SPLITS
def test_on_the_fly_gradient_passes_past_the_statistics_cap(split):
    _run_u1_family(*O.CO1_PAST_PROJ_CAP, splits=(split,))


# =================================================================================================================================
# gradient scales
# =================================================================================================================================
def _seed_inputs(npix):
    g = torch.Generator().manual_seed(npix)
    d = torch.randn(npix, generator=g) * 3e-4
    return {"random": d, "zero": torch.zeros(npix), "tiny": torch.full((npix,), 1e-30) * torch.where(torch.arange(npix) % 2 == 0, 1.0, -1.0)}


@pytest.mark.parametrize("split", [False, True], ids=["plain", "split"])
@pytest.mark.parametrize("npix", O.SEED_SIZES)
def test_gradient_seed_and_scale(npix, split):
    lib, N = _lib()
    dev = _dev()
    st = _stream(dev)
    for kind, d in _seed_inputs(npix).items():
        case = "npix%d_%s_%s" % (npix, "split" if split else "plain", kind)
        d_ = d.to(dev)
        amax_true = float(d.abs().max())
        dzb = _nan((npix, 64 if split else 32), torch.float16, dev)
        S, am = _nan((1,), torch.float32, dev), _nan((1,), torch.float32, dev)
        N.check(lib.nastar_grad_seed_f16(d_.data_ptr(), npix, int(split), dzb.data_ptr(), S.data_ptr(), am.data_ptr(), st), "seed")
        S2, am2 = _nan((1,), torch.float32, dev), _nan((1,), torch.float32, dev)
        N.check(lib.nastar_grad_scale_f32(d_.data_ptr(), npix, S2.data_ptr(), am2.data_ptr(), st), "scale")
        for entry, s, a in (("nastar_grad_seed_f16", float(S), float(am)), ("nastar_grad_scale_f32", float(S2), float(am2))):
            _exact(entry, case, a == amax_true)
            assert O.scale_window_ok(s, amax_true, -60, 60), (entry, case, s, amax_true)
            if kind == "zero":
                assert s == 1.0
            if kind == "tiny":
                assert s == 2.0 ** 60  # 1024 / 1e-30 ~ 2^109: the clamp
        ref = O.grad_seed(d, float(S), split)
        _exact("nastar_grad_seed_f16", case + "_bits", torch.equal(dzb.cpu().view(torch.int16), ref.view(torch.int16)))


@SPLITS
def test_batchnorm_backward_scale_of_a_zero_and_of_a_vanishing_gradient(split):
    """gscale_out of the BatchNorm backward (stored gradient, on-the-fly gradient, one-workgroup form): an all-zero gradient keeps the scale
    (factor 1), a vanishing one hits the clamp 2^40"""
    lib, N = _lib()
    dev = _dev()
    st = _stream(dev)
    C, shape, S_in = 16, (2, 2, 2), 8.0
    B, H, W = shape
    npix = B * H * W
    blk = _front_block(C, shape, split, 77)
    fwd = blk["fwd"]
    z_, w_ = O.nhwc(blk["z"], split).to(dev), blk["w"].to(dev)
    ms_, mt_ = blk["k2f"].to(dev), blk["k3f"].to(dev)
    mean_, invstd_ = fwd["mean"].to(dev), fwd["invstd"].to(dev)
    nb = int(lib.nastar_chan_stats_workspace_bytes(npix, C))
    tiny16 = 2.0 ** -24  # the smallest fp16 number
    for kind, dval, daval, gam in (("zero", 0.0, 0.0, 1.0), ("tiny", 1e-30, tiny16, 1e-12)):
        gamma_ = torch.full((C,), gam, device=dev)  # (a tiny gamma pushes the stored fp16 gradient's product below 2^-30; d = 1e-30 is there already)
        d_ = torch.full((B, H, W), dval, device=dev)
        da_ = O.nhwc(torch.full((B, C, H, W), daval), split).to(dev)
        want = 1.0 if kind == "zero" else 2.0 ** 40
        kmax = float((gam * fwd["invstd"]).abs().float().max())
        for entry in ("nastar_bn_stats_coef_bwd_u1_f16", "nastar_bn_stats_coef_bwd_f16", "nastar_bn_coef_bwd_io"):
            gs_in, gs_out = torch.full((1,), S_in, device=dev), _nan((1,), torch.float32, dev)
            outs = [_nan((C,), torch.float32, dev) for _ in range(5)]
            ws = _nan((nb // 4,), torch.float32, dev)
            tail = (mean_.data_ptr(), invstd_.data_ptr(), gamma_.data_ptr(), gs_in.data_ptr(), gs_out.data_ptr(), *(t.data_ptr() for t in outs))
            if entry == "nastar_bn_stats_coef_bwd_u1_f16":
                N.check(lib.nastar_bn_stats_coef_bwd_u1_f16(d_.data_ptr(), w_.data_ptr(), B, H, W, z_.data_ptr(), ms_.data_ptr(), mt_.data_ptr(), C, int(split),
                                                            *tail, None, ws.data_ptr(), nb, st), entry)
                amax = S_in * dval * float(blk["w"].abs().sum(dim=(2, 3)).max())  # an upper estimate: only its order matters for the clamp
            elif entry == "nastar_bn_stats_coef_bwd_f16":
                N.check(lib.nastar_bn_stats_coef_bwd_f16(da_.data_ptr(), z_.data_ptr(), ms_.data_ptr(), mt_.data_ptr(), npix, C, int(split), *tail, None,
                                                         ws.data_ptr(), nb, st), entry)
                amax = daval
            else:
                sums, am = _nan((C, 2), torch.float64, dev), _nan((1,), torch.float32, dev)
                N.check(lib.nastar_chan_stats_f16_ws(da_.data_ptr(), z_.data_ptr(), ms_.data_ptr(), mt_.data_ptr(), sums.data_ptr(), am.data_ptr(), npix, C,
                                                     int(split), ws.data_ptr(), nb, st), "stats ws")
                assert float(am) == daval
                N.check(lib.nastar_bn_coef_bwd_io(sums.data_ptr(), am.data_ptr(), mean_.data_ptr(), invstd_.data_ptr(), gamma_.data_ptr(), npix,
                                                  gs_in.data_ptr(), gs_out.data_ptr(), *(t.data_ptr() for t in outs), C, st), entry)
                amax = daval
            r = float(gs_out) / S_in
            _exact(entry, "scale_%s_%s" % (kind, "split" if split else "plain"), r == want and float(gs_in) == S_in)
            assert O.pow2_exponent(r) is not None and -40 <= O.pow2_exponent(r) <= 40
            assert 2.0 * kmax * amax * r <= 1024.0
            if kind == "zero":
                assert all(float(t.abs().max()) == 0.0 for t in (outs[0], outs[1], outs[3], outs[4]))  # dgamma, dbeta, c2, c3


def test_absmax_of_several_tensors():
    lib, N = _lib()
    dev = _dev()
    g = torch.Generator().manual_seed(5)
    ts = [torch.randn(n, generator=g).to(dev) for n in (1, 257, 70000)]
    ts[2][69999] = -9.5  # the maximum in the last element, negative
    table = torch.tensor([[t.data_ptr(), t.numel()] for t in ts], dtype=torch.int64).to(dev)
    scal = torch.full((3, 3), 7.0, device=dev)
    N.check(lib.nastar_absmax_multi_f32(table.data_ptr(), 3, scal.data_ptr(), _stream(dev)), "absmax multi")
    got = scal.cpu()
    for i, t in enumerate(ts):
        _exact("nastar_absmax_multi_f32", "n%d" % t.numel(), float(got[i, 2]) == float(t.abs().max()))
    # the entry point zeroes the table; the kernel touches the maxima only
    assert torch.equal(got[:, :2], torch.zeros(3, 2))


# =================================================================================================================================
# the plain BatchNorm passes (stored gradient) against float64
# =================================================================================================================================
BN_CASES = [(C, n) for C in O.BN_CHANNELS for n in O.bn_npix_cases(C)]


@pytest.mark.parametrize("split", [False, True], ids=["plain", "split"])
@pytest.mark.parametrize("C,npix", BN_CASES, ids=["C%d_npix%d" % c for c in BN_CASES])
def test_batchnorm_passes_against_float64(C, npix, split):
    lib, N = _lib()
    dev = _dev()
    st = _stream(dev)
    case = "C%d_npix%d_%s" % (C, npix, "split" if split else "plain")
    g = torch.Generator().manual_seed(3000 + C + 13 * npix)
    z = torch.randn((npix, C, 1, 1), generator=g) * 1.5 + 0.2
    da = torch.randn((npix, C, 1, 1), generator=g) * 3.0
    gamma = torch.rand(C, generator=g) + 0.5
    beta = (torch.rand(C, generator=g) * 0.3 + 0.2) * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    rm0, rv0 = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5

    def coef(v):
        f = O.bn_forward(v, gamma, beta, EPS, MOM, None, None)
        return f["k2"].float().double(), f["k3"].float().double()

    z, zs = O.deambiguate(z, split, coef)
    das = O.seen(da, split)
    fwd = O.bn_forward(zs, gamma, beta, EPS, MOM, rm0, rv0)
    fb = O.bn_forward_bounds(zs, gamma, beta, EPS, MOM, fwd)
    z_, da_ = O.nhwc(z, split).to(dev), O.nhwc(da, split).to(dev)
    gamma_, beta_ = gamma.to(dev), beta.to(dev)
    nb = int(lib.nastar_chan_stats_workspace_bytes(npix, C))
    assert nb == O.stats_grid(npix, C) * (2 * C * 8 + 4)

    # ---- forward: statistics (atomic form, two-stage form), coefficients (one-workgroup form, finish + coefficients form) ----
    s_ref = torch.stack((zs.sum(dim=(0, 2, 3)), (zs * zs).sum(dim=(0, 2, 3))), dim=1)
    s_bound = torch.stack((fb["sum0"], fb["sum1"]), dim=1)
    s_at = _nan((C, 2), torch.float64, dev)
    N.check(lib.nastar_chan_stats_f16(None, z_.data_ptr(), None, None, s_at.data_ptr(), None, npix, C, int(split), st), "stats")
    _check("nastar_chan_stats_f16", case + "_fwd", s_at, s_ref, s_bound)
    s_ws = _nan((C, 2), torch.float64, dev)
    ws = _nan((nb // 4,), torch.float32, dev)
    N.check(lib.nastar_chan_stats_f16_ws(None, z_.data_ptr(), None, None, s_ws.data_ptr(), None, npix, C, int(split), ws.data_ptr(), nb, st), "stats ws")
    _check("nastar_chan_stats_f16_ws", case + "_fwd", s_ws, s_ref, s_bound)
    forms = []
    for form in ("nastar_bn_coef_fwd", "nastar_bn_stats_coef_fwd_f16"):
        k2, k3 = _nan((C,), torch.float32, dev), _nan((C,), torch.float32, dev)
        mean, invstd = _nan((C,), torch.float64, dev), _nan((C,), torch.float64, dev)
        rm, rv = rm0.to(dev), rv0.to(dev)
        if form == "nastar_bn_coef_fwd":
            N.check(lib.nastar_bn_coef_fwd(s_ws.data_ptr(), gamma_.data_ptr(), beta_.data_ptr(), EPS, npix, MOM, rm.data_ptr(), rv.data_ptr(),
                                           k2.data_ptr(), k3.data_ptr(), mean.data_ptr(), invstd.data_ptr(), C, st), form)
            extra = s_ws
        else:
            ws = _nan((nb // 4,), torch.float32, dev)
            extra = _nan((C, 2), torch.float64, dev)
            N.check(lib.nastar_bn_stats_coef_fwd_f16(z_.data_ptr(), npix, C, int(split), gamma_.data_ptr(), beta_.data_ptr(), EPS, MOM, rm.data_ptr(),
                                                     rv.data_ptr(), k2.data_ptr(), k3.data_ptr(), mean.data_ptr(), invstd.data_ptr(), extra.data_ptr(),
                                                     ws.data_ptr(), nb, st), form)
        res = dict(k2=k2, k3=k3, mean=mean, invstd=invstd, rm=rm, rv=rv)
        for name, t in res.items():
            _check(form, case + "_" + name, t, fwd[name], fb[name])
        forms.append(list(res.values()) + [extra])
    _exact("nastar_bn_stats_coef_fwd_f16", case + "_bits", all(torch.equal(a, b) for a, b in zip(*forms)))
    k2_, k3_ = forms[0][0], forms[0][1]
    k2k, k3k = k2_.double().cpu(), k3_.double().cpu()
    out = _nan(tuple(z_.shape), torch.float16, dev)
    N.check(lib.nastar_chan_affine_f16(None, z_.data_ptr(), None, k2_.data_ptr(), k3_.data_ptr(), None, None, out.data_ptr(), npix, C, 1, int(split), st),
            "affine fwd")
    ref = torch.relu(O._cvec(k2k) * zs + O._cvec(k3k))
    zero = torch.zeros(C, dtype=torch.float64)
    bound = O.affine_bound(zero, 0.0, k2k, zs, k3k, split)  # (the store bound of the value before the ReLU covers the one after)
    _check("nastar_chan_affine_f16", case + "_fwd", O.from_nhwc(out, C, split), ref, bound, O.N_AFFINE)

    # ---- backward: the ReLU mask of the kernel's own k2 / k3, three launch forms ----
    assert int(O.mask_ambiguous(zs, k2k, k3k).sum()) == 0
    mask = ((O._cvec(k2k) * zs + O._cvec(k3k)) > 0).double()
    dy = das * mask
    bwd = O.bn_backward(zs, dy, gamma, fwd)
    bb = O.bn_backward_bounds(zs, dy, torch.zeros_like(dy), gamma, fwd, bwd)
    S_in = 4.0
    mean_, invstd_ = fwd["mean"].to(dev), fwd["invstd"].to(dev)
    sb_ref, sb_bound = torch.stack((bwd["sdy"], bwd["sdyz"]), dim=1), torch.stack((bb["sdy"], bb["sdyz"]), dim=1)
    amax_ref = float(dy.abs().max().float())
    s_at, a_at = _nan((C, 2), torch.float64, dev), _nan((1,), torch.float32, dev)
    N.check(lib.nastar_chan_stats_f16(da_.data_ptr(), z_.data_ptr(), k2_.data_ptr(), k3_.data_ptr(), s_at.data_ptr(), a_at.data_ptr(), npix, C,
                                      int(split), st), "stats bwd")
    _check("nastar_chan_stats_f16", case + "_bwd", s_at, sb_ref, sb_bound)
    _exact("nastar_chan_stats_f16", case + "_amax", float(a_at) == amax_ref)
    s_ws, a_ws = _nan((C, 2), torch.float64, dev), _nan((1,), torch.float32, dev)
    ws = _nan((nb // 4,), torch.float32, dev)
    N.check(lib.nastar_chan_stats_f16_ws(da_.data_ptr(), z_.data_ptr(), k2_.data_ptr(), k3_.data_ptr(), s_ws.data_ptr(), a_ws.data_ptr(), npix, C,
                                         int(split), ws.data_ptr(), nb, st), "stats ws bwd")
    _check("nastar_chan_stats_f16_ws", case + "_bwd", s_ws, sb_ref, sb_bound)
    _exact("nastar_chan_stats_f16_ws", case + "_amax", float(a_ws) == amax_ref)
    kmax = float((gamma.double() * fwd["invstd"]).abs().max())
    forms = []
    for form in ("nastar_bn_coef_bwd", "nastar_bn_coef_bwd_io", "nastar_bn_stats_coef_bwd_f16"):
        dgamma, dbeta, c1, c2, c3 = (_nan((C,), torch.float32, dev) for _ in range(5))
        gs_in, gs_out = torch.full((1,), S_in, device=dev), _nan((1,), torch.float32, dev)
        tail = (dgamma.data_ptr(), dbeta.data_ptr(), c1.data_ptr(), c2.data_ptr(), c3.data_ptr())
        if form == "nastar_bn_coef_bwd":
            N.check(lib.nastar_bn_coef_bwd(s_ws.data_ptr(), a_ws.data_ptr(), mean_.data_ptr(), invstd_.data_ptr(), gamma_.data_ptr(), npix,
                                           gs_in.data_ptr(), *tail, C, st), form)
            gs_out = gs_in  # in place
        elif form == "nastar_bn_coef_bwd_io":
            N.check(lib.nastar_bn_coef_bwd_io(s_ws.data_ptr(), a_ws.data_ptr(), mean_.data_ptr(), invstd_.data_ptr(), gamma_.data_ptr(), npix,
                                              gs_in.data_ptr(), gs_out.data_ptr(), *tail, C, st), form)
            assert float(gs_in) == S_in
        else:
            ws = _nan((nb // 4,), torch.float32, dev)
            so = _nan((C, 2), torch.float64, dev)
            N.check(lib.nastar_bn_stats_coef_bwd_f16(da_.data_ptr(), z_.data_ptr(), k2_.data_ptr(), k3_.data_ptr(), npix, C, int(split),
                                                     mean_.data_ptr(), invstd_.data_ptr(), gamma_.data_ptr(), gs_in.data_ptr(), gs_out.data_ptr(), *tail,
                                                     so.data_ptr(), ws.data_ptr(), nb, st), form)
            assert float(gs_in) == S_in and torch.equal(so, s_ws)
        r = float(gs_out) / S_in
        assert O.scale_window_ok(r, 2.0 * kmax * amax_ref, -40, 40), (form, case, r, kmax, amax_ref)
        _check(form, case + "_dgamma", dgamma.double().cpu() * S_in, bwd["dgamma"], bb["dgamma"])
        _check(form, case + "_dbeta", dbeta.double().cpu() * S_in, bwd["dbeta"], bb["dbeta"])
        for name, t in (("c1", c1), ("c2", c2), ("c3", c3)):
            _check(form, case + "_" + name, t.double().cpu() / r, bwd[name], bb[name])
        forms.append([dgamma, dbeta, c1, c2, c3, gs_out.clone()])
    _exact("nastar_bn_stats_coef_bwd_f16", case + "_bits", all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(*forms)))
    # ---- dz: against the kernel's own coefficients, then against float64 autograd of BatchNorm + ReLU ----
    dgamma, dbeta, c1, c2, c3, gs_out = forms[2]
    r = float(gs_out) / S_in
    out = _nan(tuple(z_.shape), torch.float16, dev)
    N.check(lib.nastar_chan_affine_f16(da_.data_ptr(), z_.data_ptr(), c1.data_ptr(), c2.data_ptr(), c3.data_ptr(), k2_.data_ptr(), k3_.data_ptr(),
                                       out.data_ptr(), npix, C, 0, int(split), st), "affine bwd")
    got = O.from_nhwc(out, C, split)
    k = [t.double().cpu() for t in (c1, c2, c3)]
    ref = O._cvec(k[0]) * dy + O._cvec(k[1]) * zs + O._cvec(k[2])
    _check("nastar_chan_affine_f16", case + "_bwd", got, ref, O.affine_bound(k[0], dy.abs(), k[1], zs, k[2], split, u=dy), O.N_AFFINE)
    if npix > 1:
        _, dz_true, dg_true, db_true = O.bn_relu_autograd(zs, gamma, beta, EPS, das)
        _check("nastar_bn_stats_coef_bwd_f16", case + "_dgamma_autograd", dgamma.double().cpu() * S_in, dg_true, bb["dgamma"] + 2.0 ** -40 * dg_true.abs())
        _check("nastar_bn_stats_coef_bwd_f16", case + "_dbeta_autograd", dbeta.double().cpu() * S_in, db_true, bb["dbeta"] + 2.0 ** -40 * db_true.abs())
    else:
        dz_true = bwd["dz"]  # one pixel: the closed form (dz = 0: the batch mean removes the only pixel)
        assert float(dz_true.abs().max()) <= 1e-9
    rc = [r * bwd[x] for x in ("c1", "c2", "c3")]
    bound = O.affine_bound(rc[0], dy.abs(), rc[1], zs, rc[2], split, coef_bounds=[r * bb[x] for x in ("c1", "c2", "c3")], u=dy)
    _check("nastar_chan_affine_f16", case + "_dz", got, r * dz_true, bound + 2.0 ** -40 * r * bwd["dz"].abs(), O.N_AFFINE)


# =================================================================================================================================
# plumbing: pooling backward, upsampling + concatenation, the scaled sum of two gradients
# =================================================================================================================================
@pytest.mark.parametrize("split", [False, True], ids=["plain", "split"])
@pytest.mark.parametrize("C1,C2", O.PLUMB_CHANNELS)
@pytest.mark.parametrize("shape", O.PLUMB_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_upsampling_concatenation_and_its_backward(shape, C1, C2, split):
    lib, N = _lib()
    dev = _dev()
    st = _stream(dev)
    B, H, W = shape
    C, M = C1 + C2, (2 if split else 1)
    case = "%dx%dx%d_c%d_%d_%s" % (B, H, W, C1, C2, "split" if split else "plain")
    g = torch.Generator().manual_seed(40 + B * H + C)
    x = torch.randn((B, C1, H // 2, W // 2), generator=g)
    sk = torch.randn((B, C2, H, W), generator=g) if C2 else None
    x_ = O.nhwc(x, split).to(dev)
    sk_ = O.nhwc(sk, split).to(dev) if C2 else None  # c2 == 0: a NULL skip pointer
    cat = _nan((B, H, W, C * M), torch.float16, dev)
    N.check(lib.nastar_upcat_f16(x_.data_ptr(), _ptr(sk_), cat.data_ptr(), B, H, W, C1, C2, int(split), st), "upcat")
    ref = O.upcat(O.seen(x, split), O.seen(sk, split) if C2 else None)
    _exact("nastar_upcat_f16", case, torch.equal(O.from_nhwc(cat, C, split), ref))
    d = torch.randn((B, C, H, W), generator=g)
    d_ = O.nhwc(d, split).to(dev)
    dx = _nan((B, H // 2, W // 2, C1 * M), torch.float16, dev)
    dsk = _nan((B, H, W, C2 * M), torch.float16, dev) if C2 else None
    N.check(lib.nastar_upcat_bwd_f16(d_.data_ptr(), dx.data_ptr(), _ptr(dsk), B, H, W, C1, C2, int(split), st), "upcat bwd")
    rx, bx, rs = O.upcat_bwd(O.seen(d, split), C1, split)
    _check("nastar_upcat_bwd_f16", case, O.from_nhwc(dx, C1, split), rx, bx, O.N_UPSUM)
    if C2:
        _exact("nastar_upcat_bwd_f16", case + "_skip", torch.equal(O.from_nhwc(dsk, C2, split), rs))


@pytest.mark.parametrize("split", [False, True], ids=["plain", "split"])
@pytest.mark.parametrize("C", O.POOL_CHANNELS)
@pytest.mark.parametrize("shape", O.PLUMB_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_scaled_sum_of_two_gradients(shape, C, split):
    lib, N = _lib()
    dev = _dev()
    B, H, W = shape
    case = "%dx%dx%d_c%d_%s" % (B, H, W, C, "split" if split else "plain")
    g = torch.Generator().manual_seed(50 + B * W + C)
    a = torch.randn((B, C, H, W), generator=g) * 300
    b = torch.randn((B, C, H, W), generator=g) * 20
    a_, b_ = O.nhwc(a, split).to(dev), O.nhwc(b, split).to(dev)
    for Sa, Sb in ((1024.0, 64.0), (2.0 ** -3, 2.0 ** 5), (16.0, 16.0)):
        Sa_, Sb_, So_ = torch.tensor([Sa], device=dev), torch.tensor([Sb], device=dev), _nan((1,), torch.float32, dev)
        out = _nan(tuple(a_.shape), torch.float16, dev)
        N.check(lib.nastar_grad_add_f16(a_.data_ptr(), Sa_.data_ptr(), b_.data_ptr(), Sb_.data_ptr(), out.data_ptr(), So_.data_ptr(), B * H * W, C,
                                        int(split), _stream(dev)), "grad add")
        ref, bound, So = O.grad_add(O.seen(a, split), Sa, O.seen(b, split), Sb, split)
        assert float(So_) == So
        _check("nastar_grad_add_f16", case + "_%g_%g" % (Sa, Sb), O.from_nhwc(out, C, split), ref, bound, O.N_GRADADD)


def _pool_batches(B, C, H, W, split, g):
    """three constructed batches of pool inputs r [B,C,H,W] (float32; seen exactly as built)"""
    h, w = H // 2, W // 2
    up = lambda t: t.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)  # noqa: E731
    pos = torch.zeros((B, C, H, W))
    pos[:, :, 1::2, :] += 2
    pos[:, :, :, 1::2] += 1  # 0..3: the place of a pixel in its window, row-major
    out = {"all_equal": up(torch.randint(0, 64, (B, C, h, w), generator=g).float() / 16)}
    want = up(torch.arange(B * C * h * w).view(B, C, h, w) % 4).float()
    out["each_position"] = (torch.rand((B, C, H, W), generator=g) + 2.0 * (pos == want).float()).to(torch.float16).float()
    if split:
        base = up(1.0 + torch.randint(0, 512, (B, C, h, w), generator=g).float() / 1024)  # fp16 numbers in [1, 1.5): spacing 2^-10
        lo = torch.randint(0, 4, (B, C, H, W), generator=g).float() * 2.0 ** -16          # below half a spacing: hi is `base` in every window
        out["hi_equal_lo_decides"] = base + lo
    return out


@pytest.mark.parametrize("split", [False, True], ids=["plain", "split"])
@pytest.mark.parametrize("C", O.POOL_CHANNELS)
@pytest.mark.parametrize("shape", O.PLUMB_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_maxpool_backward_tie_rules(shape, C, split):
    lib, N = _lib()
    dev = _dev()
    B, H, W = shape
    g = torch.Generator().manual_seed(60 + B * H + C)
    dp = torch.randn((B, C, H // 2, W // 2), generator=g)
    dp_ = O.nhwc(dp, split).to(dev)
    for kind, r in _pool_batches(B, C, H, W, split, g).items():
        case = "%dx%dx%d_c%d_%s_%s" % (B, H, W, C, "split" if split else "plain", kind)
        rs = O.seen(r, split)
        assert torch.equal(rs, r.double()), "the constructed values must be seen exactly"
        if kind == "hi_equal_lo_decides":
            hi = r.to(torch.float16).double().view(B, C, H // 2, 2, W // 2, 2)
            assert torch.equal(hi.amax(dim=(3, 5)), hi.amin(dim=(3, 5))) and not torch.equal(rs, r.to(torch.float16).double())
        r_ = O.nhwc(r, split).to(dev)
        dr = _nan(tuple(r_.shape), torch.float16, dev)
        N.check(lib.nastar_maxpool2x2_bwd_f16(r_.data_ptr(), dp_.data_ptr(), dr.data_ptr(), B, H, W, C, int(split), _stream(dev)), "pool bwd")
        got = O.from_nhwc(dr, C, split)
        rr = rs.clone().requires_grad_(True)
        F.max_pool2d(rr, 2).backward(O.seen(dp, split))
        _exact("nastar_maxpool2x2_bwd_f16", case, torch.equal(got, rr.grad) and torch.equal(got, O.maxpool_bwd(rs, O.seen(dp, split))))
