"""tests/encoder_stream_oracle.py on its own (no device): its closed forms against torch float64 autograd, and its comparison routine
against deliberately wrong results -- the proof that tests/test_encoder_stream_edges_gpu.py can fail.  Every defect is applied to the
oracle's own output at the GPU tests' shapes and must exceed the bound the GPU result is held to; the shapes at which a defect changes
nothing are named next to it and asserted to be exactly those."""
import pytest
import torch
import torch.nn.functional as F

import encoder_stream_oracle as O

EPS, MOM = 1e-5, 0.1
CO1_CASES = [(C, s) for C in O.CO1_CHANNELS for s in O.CO1_SHAPES] + [O.CO1_PAST_PROJ_CAP]
U1_CASES = [(C, s) for C in O.U1_CHANNELS for s in O.CO1_SHAPES] + [O.CO1_PAST_PROJ_CAP]
BN_CASES = [(C, n) for C in O.BN_CHANNELS for n in O.bn_npix_cases(C)]
_id = lambda c: "C%d_%s" % (c[0], "x".join(str(v) for v in c[1]) if isinstance(c[1], tuple) else "npix%d" % c[1])  # noqa: E731


def _close(a, b, scale):
    """two float64 evaluations of one quantity: within the double-sum rtol of the sum of absolute terms"""
    return O.ratio(a, b, O.DSUM_RTOL * scale) <= 1.0


def _block(C, shape, split, seed=0):
    B, H, W = shape
    g = torch.Generator().manual_seed(100 + seed + C + 7 * B * H * W)
    z = torch.randn((B, C, H, W), generator=g) * 1.5 + 0.2
    gamma = torch.rand(C, generator=g) + 0.5
    beta = (torch.rand(C, generator=g) * 0.3 + 0.2) * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)

    def coef(v):
        f = O.bn_forward(v, gamma, beta, EPS, MOM, None, None)
        return f["k2"].float().double(), f["k3"].float().double()

    z, zs = O.deambiguate(z, split, coef)
    fwd = O.bn_forward(zs, gamma, beta, EPS, MOM, None, None)
    k2, k3 = coef(zs)
    assert int(O.mask_ambiguous(zs, k2, k3).sum()) == 0
    return dict(zs=zs, gamma=gamma, beta=beta, fwd=fwd, k2=k2, k3=k3,
                a=O.seen(torch.relu(torch.randn((B, C, H, W), generator=g)), split),
                w=torch.randn((1, C, 3, 3), generator=g) * 0.1, bias=torch.randn(1, generator=g), d=torch.randn((B, H, W), generator=g))


# ---- closed forms against float64 autograd ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", O.CO1_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_closing_convolution_gradients_are_autograd(shape):
    C = 16
    blk = _block(C, shape, True)
    for k2, k3 in ((None, None), (blk["k2"], blk["k3"])):
        src = blk["a"] if k2 is None else blk["zs"]
        x = O.co1_input(src, k2, k3)[0].clone().requires_grad_(True)
        w = blk["w"].double().clone().requires_grad_(True)
        z = F.conv2d(x, w, blk["bias"].double(), padding=1)
        z.backward(blk["d"].double()[:, None])
        ref_z, bound = O.co1_forward(src, blk["w"], blk["bias"], O.n_conv(C, k2 is not None), k2, k3)
        assert torch.equal(ref_z, z.detach()[:, 0]) and bool((bound > 0).all())
        dw, bw = O.co1_wgrad(blk["d"], src, 1, k2, k3)
        assert _close(dw, w.grad, bw / O.U24)
        u, bu = O.co1_u1(blk["d"], blk["w"], 8.0, x.shape)
        assert _close(u, 8.0 * x.grad, bu / (O.N_U1 * O.U24))


@pytest.mark.parametrize("C,npix", BN_CASES, ids=[_id(c) for c in BN_CASES])
def test_batchnorm_closed_forms_are_autograd(C, npix):
    g = torch.Generator().manual_seed(C + npix)
    z = O.seen(torch.randn((npix, C, 1, 1), generator=g) * 1.5 + 0.2, True)
    da = O.seen(torch.randn((npix, C, 1, 1), generator=g) * 3, True)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    rm, rv = torch.randn(C, generator=g).double() * 0.1, torch.rand(C, generator=g).double() + 0.5
    fwd = O.bn_forward(z, gamma, beta, EPS, MOM, rm, rv)
    a = torch.relu(O._cvec(fwd["k2"]) * z + O._cvec(fwd["k3"]))
    dy = da * (a > 0)
    bwd = O.bn_backward(z, dy, gamma, fwd)
    if npix == 1:  # torch refuses batch statistics of one pixel: variance 0, unbiased factor taken as 1, and the mean removes the whole gradient
        assert torch.equal(fwd["mean"], z[0, :, 0, 0]) and float(fwd["var"].abs().max()) == 0.0
        assert _close(fwd["rv"], (1 - MOM) * rv, rv) and _close(fwd["rm"], (1 - MOM) * rm + MOM * z[0, :, 0, 0], rm.abs() + 1)
        assert _close(a[0, :, 0, 0], torch.relu(beta.double()), 1e4 * (1 + z[0, :, 0, 0].abs()))  # k3 = beta - mean k2 cancels at invstd = 316
        assert float(bwd["dz"].abs().max()) <= 1e-9 and float(bwd["dgamma"].abs().max()) <= 1e-9
        with pytest.raises(AssertionError):
            O.bn_relu_autograd(z, gamma, beta, EPS, da)
        return
    rm_t, rv_t = rm.clone(), rv.clone()
    a_t = torch.relu(F.batch_norm(z, rm_t, rv_t, gamma.double(), beta.double(), True, MOM, EPS))
    scale = 1 + z.abs().max() * fwd["invstd"].max()
    assert _close(a, a_t, 1e2 * scale) and _close(fwd["rm"], rm_t, 1e2) and _close(fwd["rv"], rv_t, 1e2 * (1 + fwd["var"]))
    _, dz_t, dg_t, db_t = O.bn_relu_autograd(z, gamma, beta, EPS, da)
    big = 1e3 * scale ** 2 * (1 + da.abs().max()) * npix
    assert _close(bwd["dz"], dz_t, big) and _close(bwd["dgamma"], dg_t, big) and _close(bwd["dbeta"], db_t, big)


@pytest.mark.parametrize("shape", O.PLUMB_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_pooling_and_upsampling_closed_forms_are_autograd(shape):
    B, H, W = shape
    g = torch.Generator().manual_seed(B * H + W)
    for C1, C2 in O.PLUMB_CHANNELS:
        x = torch.randn((B, C1, H // 2, W // 2), generator=g).double().requires_grad_(True)
        sk = torch.randn((B, C2, H, W), generator=g).double().requires_grad_(True) if C2 else None
        up = F.interpolate(x, scale_factor=2, mode="nearest")
        cat = up if sk is None else torch.cat((up, sk), dim=1)
        assert torch.equal(O.upcat(x.detach(), None if sk is None else sk.detach()), cat.detach())
        d = torch.randn(cat.shape, generator=g).double()
        cat.backward(d)
        dx, bx, ds = O.upcat_bwd(d, C1, True)
        assert _close(dx, x.grad, bx / O.U24) and (sk is None or torch.equal(ds, sk.grad))
    for C in O.POOL_CHANNELS:
        r = torch.randint(0, 3, (B, C, H, W), generator=g).double().requires_grad_(True)  # three values: ties in most windows
        dp = torch.randn((B, C, H // 2, W // 2), generator=g).double()
        F.max_pool2d(r, 2).backward(dp)
        assert torch.equal(O.maxpool_bwd(r.detach(), dp), r.grad)
    a, b = torch.randn(5, generator=g).double(), torch.randn(5, generator=g).double()
    out, _, So = O.grad_add(a, 1024.0, b, 64.0, False)
    assert So == 64.0 and torch.equal(out, a / 16 + b)


def test_comparison_routine_and_scale_rules():
    one = torch.ones(3, dtype=torch.float64)
    assert O.ratio(one, one, 0 * one) == 0.0 and O.ratio(one + 1e-9, one, 0 * one) == O.INF
    assert O.ratio(torch.tensor([1.0, float("nan")]), torch.ones(2), torch.ones(2)) == O.INF  # an unwritten sentinel
    assert abs(O.ratio(one + 0.5, one, 0.25 * one) - 2.0) < 1e-12
    assert O.pow2_exponent(1.0) == 0 and O.pow2_exponent(2.0 ** -40) == -40 and O.pow2_exponent(3.0) is None and O.pow2_exponent(0.0) is None
    assert O.scale_window_ok(1.0, 0.0, -60, 60) and not O.scale_window_ok(2.0, 0.0, -60, 60)
    assert O.scale_window_ok(2.0 ** 60, 1e-30, -60, 60) and not O.scale_window_ok(2.0 ** 61, 1e-30, -60, 60)
    assert O.scale_window_ok(1024.0, 1.0, -60, 60) and O.scale_window_ok(256.0, 3.0, -60, 60)
    assert not O.scale_window_ok(512.0, 0.99, -60, 60) and not O.scale_window_ok(2048.0, 1.0, -60, 60) and not O.scale_window_ok(768.0, 1.0, -60, 60)
    # the geometry the bounds' n come from
    assert (O.npl(8), O.npl(512), O.npl(2048)) == (256, 4, 1)
    assert O.n_conv(256, False) == 8 + 5 + 9 and O.n_conv(8, True) == 8 + 0 + 9 + 2
    assert O.n_wgrad(105, 128, False) == 7 + 16 + 1 and O.n_wgrad(33792, 512, False) == 9 + 4 + 1
    assert O.stats_grid(33792, 512) == 1024 and O.stats_grid(4097, 2048) == 1024 and O.stats_grid(4096, 2048) == 1024 and O.stats_grid(105, 8) == 1
    d = torch.tensor([0.5, -3.0, 0.0])
    s = O.grad_seed(d, 256.0, True)
    assert s.shape == (3, 64) and float(s[1, 0]) == -768.0 and float(s[:, 1:32].abs().max()) == 0.0 and float(s[:, 33:].abs().max()) == 0.0


def test_generators_leave_no_ambiguous_relu_decision():
    z = torch.tensor([[[[1.0]], [[0.0]], [[-2.0]]]])  # ms*v + mt = 0 exactly in channels 0 and 2; channel 1 has both terms zero
    ms, mt = torch.tensor([2.0, 1.0, 1.0]).double(), torch.tensor([-2.0, 0.0, 2.0]).double()
    assert O.mask_ambiguous(z.double(), ms, mt).view(-1).tolist() == [True, False, True]
    fixed, fixed_seen = O.deambiguate(z, True, lambda v: (ms, mt))
    assert torch.equal(fixed_seen, O.seen(fixed, True)) and int(O.mask_ambiguous(fixed_seen, ms, mt).sum()) == 0 and float(fixed[0, 1]) == 0.0
    with pytest.raises(AssertionError):
        O.deambiguate(z, True, lambda v: (0 * ms + 1, -v.view(-1)))  # a decision no replacement can move


# ---- the defects -----------------------------------------------------------------------------------------------------------------------------
def _flat(t):  # [B,C,H,W] -> [npix, C] in the kernels' pixel order
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _unflat(f, shape):
    B, C, H, W = shape
    return f.view(B, H, W, C).permute(0, 3, 1, 2).contiguous()


def _shift_unguarded(P, W):
    """z[q] = sum_tap P[q + off(tap)][tap] over the FLAT pixel array [npix, 9] with no image border: a tap outside its image reads the
    neighbouring row or image (zero only outside the array)"""
    n = P.shape[0]
    z = torch.zeros(n, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            off = (ky - 1) * W + (kx - 1)
            src = torch.arange(n) + off
            ok = (src >= 0) & (src < n)
            z[ok] += P[src[ok], ky * 3 + kx]
    return z


def _taps_unguarded(d, W):
    """s[p][tap] = d[p - off(tap)] over the flat array, no image border"""
    n = d.numel()
    s = torch.zeros((n, 9), dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            src = torch.arange(n) - ((ky - 1) * W + (kx - 1))
            ok = (src >= 0) & (src < n)
            s[ok, ky * 3 + kx] = d.reshape(-1)[src[ok]]
    return s


def _mirror_tap(w):
    """tap (ky, kx) = (1, 0) read at x + 1 instead of x - 1"""
    w = w.clone()
    w[..., 1, 2] += w[..., 1, 0]
    w[..., 1, 0] = 0
    return w


def _lane_twice(a):
    """channels 0..7 of the next pixel (the neighbouring pixel lane) added once more"""
    f = _flat(a).clone()
    f[:-1, :8] += f[1:, :8].clone()
    return _unflat(f, a.shape)


def _swap_hw(t):
    return t.reshape(t.shape[:-2] + (t.shape[-1], t.shape[-2]))


@pytest.mark.parametrize("C,shape", CO1_CASES, ids=[_id(c) for c in CO1_CASES])
def test_defects_of_the_closing_convolution_are_rejected(C, shape):
    B, H, W = shape
    npix = B * H * W
    blk = _block(C, shape, False, seed=1)
    a, w, bias, d = blk["a"], blk["w"].double(), blk["bias"], blk["d"].double()
    n = O.n_conv(C, False)
    z, bz = O.co1_forward(a, w, bias, n)
    fwd = lambda aa, ww: O.co1_forward(aa, ww, bias, n)[0]  # noqa: E731
    P = _flat(a) @ w[0].reshape(C, 9)
    rejected = {
        # a border tap read from the neighbouring row / image instead of zero (in a one-pixel-wide image, taps (0,2) and (2,0) then read the pixel itself)
        "border": (lambda: O.ratio((_shift_unguarded(P, W) + bias.double()).view(B, H, W), z, bz), True),
        # H and W exchanged: the same image when it is square
        "swap_hw": (lambda: O.ratio(_swap_hw(fwd(_swap_hw(a), w)), z, bz), H != W),
        # one tap mirrored: both its places lie outside a one-pixel-wide image
        "mirror": (lambda: O.ratio(fwd(a, _mirror_tap(w)), z, bz), W > 1),
        # channels 0..7 of the neighbouring pixel lane added once more: a single pixel has no neighbour
        "lane_twice": (lambda: O.ratio(fwd(_lane_twice(a), w), z, bz), npix > 1),
    }
    nw = O.n_wgrad(npix, C, False)
    dw, bw = O.co1_wgrad(d, a, nw)
    wg = lambda dd, aa: torch.nn.grad.conv2d_weight(aa, (1, C, 3, 3), dd[:, None], padding=1)  # noqa: E731
    last = a.clone()
    last[-1, :, -1, -1] = 0
    rejected.update({
        "wgrad_last_pixel": (lambda: O.ratio(wg(d, last), dw, bw), True),
        "wgrad_border": (lambda: O.ratio((_flat(a).t() @ _taps_unguarded(d, W)).view(1, C, 3, 3), dw, bw), True),
        "wgrad_swap_hw": (lambda: O.ratio(wg(_swap_hw(d), _swap_hw(a)), dw, bw), H != W),
        "wgrad_lane_twice": (lambda: O.ratio(wg(d, _lane_twice(a)), dw, bw), npix > 1),
    })
    for name, (r, applies) in rejected.items():
        if not applies and npix > 10000:
            continue  # (the large case is square: H <-> W is the same image, as asserted at (2,2,2))
        r = r()
        assert (r > 1.0) if applies else (r <= 1.0), (name, r, applies)


def _unpaired(npix, C):
    """pixels the statistics kernel meets with no partner: lane start q (< step), pixels q, q + step, ... taken two at a time"""
    step = O.stats_grid(npix, C) * O.npl(C)
    p = torch.arange(npix)
    return p[((p // step) % 2 == 0) & (p + step >= npix)]


# the cases that leave no pixel without a partner (every lane that has a pixel has an even number of them): there "the unpaired tail pixel
# counted twice" changes nothing
ALL_PAIRED = {(2048, 2)}
ALL_PAIRED_U1 = {(512, (2, 2, 2)), (512, (2, 3, 40)), (512, (2, 40, 3)), (1024, (2, 2, 2)), (1024, (2, 3, 40)), (1024, (2, 40, 3))}


@pytest.mark.parametrize("C,npix", BN_CASES, ids=[_id(c) for c in BN_CASES])
def test_defects_of_the_statistics_are_rejected(C, npix):
    blk = _block(C, (npix, 1, 1), True, seed=2)
    zs, fwd, gamma = blk["zs"], blk["fwd"], blk["gamma"]
    fb = O.bn_forward_bounds(zs, gamma, blk["beta"], EPS, MOM, fwd)
    g = torch.Generator().manual_seed(npix)
    dy = O.seen(torch.randn(zs.shape, generator=g) * 3, True) * ((O._cvec(blk["k2"]) * zs + O._cvec(blk["k3"])) > 0)
    bwd = O.bn_backward(zs, dy, gamma, fwd)
    bb = O.bn_backward_bounds(zs, dy, torch.zeros_like(dy), gamma, fwd, bwd)
    tail = _unpaired(npix, C)
    assert (tail.numel() == 0) == ((C, npix) in ALL_PAIRED)
    for name, keep in (("last_pixel", None), ("tail_twice", tail)):
        if keep is None:
            f = lambda t: t[:-1].sum(dim=(0, 2, 3))  # noqa: E731
        else:
            f = lambda t: t.sum(dim=(0, 2, 3)) + t[keep].sum(dim=(0, 2, 3))  # noqa: E731
        rs = [O.ratio(f(zs), zs.sum(dim=(0, 2, 3)), fb["sum0"]), O.ratio(f(zs * zs), (zs * zs).sum(dim=(0, 2, 3)), fb["sum1"]),
              O.ratio(f(dy), bwd["sdy"], bb["sdy"]), O.ratio(f(dy * zs), bwd["sdyz"], bb["sdyz"])]
        if name == "tail_twice" and tail.numel() == 0:
            assert max(rs) == 0.0
        else:
            assert min(rs) > 1.0, (name, rs)
        # ... and the coefficients computed from such sums leave their bounds too
        if name == "last_pixel" and npix > 1:
            bad = O.bn_backward(zs, torch.cat((dy[:-1], 0 * dy[-1:])), gamma, fwd)
            assert all(O.ratio(bad[k], bwd[k], bb[k]) > 1.0 for k in ("dgamma", "dbeta", "c2", "c3"))


@pytest.mark.parametrize("C,shape", U1_CASES, ids=[_id(c) for c in U1_CASES])
def test_defects_of_the_on_the_fly_gradient_are_rejected(C, shape):
    B, H, W = shape
    npix = B * H * W
    blk = _block(C, shape, False, seed=3)
    zs, fwd, gamma, w, d = blk["zs"], blk["fwd"], blk["gamma"], blk["w"].double(), blk["d"].double()
    full = (B, C, H, W)
    u, e_u = O.co1_u1(d, w, 8.0, full)
    mask = ((O._cvec(blk["k2"]) * zs + O._cvec(blk["k3"])) > 0).double()
    dy, e_dy = u * mask, e_u * mask
    bwd = O.bn_backward(zs, dy, gamma, fwd)
    bb = O.bn_backward_bounds(zs, dy, e_dy, gamma, fwd, bwd)
    S_dy = e_dy / (O.N_U1 * O.U24)
    dz_bound = None if npix > 10000 else O.affine_bound(bwd["c1"], S_dy, bwd["c2"], zs, bwd["c3"], False, n_u=O.N_U1, coef_bounds=[bb[k] for k in ("c1", "c2", "c3")], u=dy)

    small = npix <= 10000  # the large case judges the sums only (dz is per pixel: its defects show at every small shape)

    def rejected(uu):
        y = uu * mask
        r = [O.ratio(y.sum(dim=(0, 2, 3)), bwd["sdy"], bb["sdy"]), O.ratio((y * zs).sum(dim=(0, 2, 3)), bwd["sdyz"], bb["sdyz"])]
        if small:
            r.append(O.ratio(O._cvec(bwd["c1"]) * y + O._cvec(bwd["c2"]) * zs + O._cvec(bwd["c3"]), bwd["dz"], dz_bound))
        return r

    assert max(rejected(u)) <= 1.0
    u_border = 8.0 * _unflat(_taps_unguarded(d, W) @ w[0].reshape(C, 9).t(), full)
    u_swap = _swap_hw(O.co1_u1(_swap_hw(d), w, 8.0, (B, C, W, H))[0]) if (H != W or small) else u
    u_mirror = O.co1_u1(d, _mirror_tap(w), 8.0, full)[0]
    tail = _unpaired(npix, C)
    twice = torch.zeros(npix, dtype=torch.float64)
    twice[tail] = 1
    u_twice = u * (1 + twice.view(B, 1, H, W))
    last = torch.ones(npix, dtype=torch.float64)
    last[-1] = 0
    u_last = u * last.view(B, 1, H, W)
    # mirrored tap: both its places lie outside a one-pixel-wide image; H <-> W: square images are the same image
    for name, uu, applies in (("border", u_border, True), ("swap_hw", u_swap, H != W), ("mirror", u_mirror, W > 1)):
        r = rejected(uu)
        assert (min(r) > 1.0) if applies else (max(r) <= 1.0), (name, r, applies)
    # the sums lose / double a pixel (dz, written per pixel, is not a sum: only the first two count)
    assert (tail.numel() == 0) == ((C, shape) in ALL_PAIRED_U1)
    for name, uu, applies in (("last_pixel", u_last, True), ("tail_twice", u_twice, tail.numel() > 0)):
        r = rejected(uu)[:2]
        assert (min(r) > 1.0) if applies else (max(r) == 0.0), (name, r)
