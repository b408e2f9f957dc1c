"""Float64 definitions of the encoder's streaming training kernels (csrc/nastar_encoder_train.hip.h, csrc/nastar_encoder_co1.hip.h), with an
error bound for every output.  No GPU, nothing from the kernels: the operations are written as the reference's modules define them
(planner/encoder.py: Conv2d(C, 1, 3, padding=1), BatchNorm2d in training mode + ReLU, MaxPool2d(2), nearest x2 upsampling + concatenation)
under torch float64 autograd.

Operands are what a kernel sees: an fp16 tensor (``hi``) or the split pair ``hi + lo`` (exact in fp32), see ``seen`` / ``nhwc``.

Bounds.  No tolerance constant is chosen here.  An output that is a sum accumulated in fp32 is held to ``n * 2^-24 * S``: ``S`` is the same
float64 operation applied to the absolute values of the operands and ``n`` the longest chain of fp32 roundings the output passes through,
taken from the launch geometry (the ``n_*`` functions below say where every term comes from).  Sums the kernels carry in double are held
to ``1e-12 * S`` (the rtol of tests/test_encoder_train_gpu.py::test_chan_stats_and_affine, applied to the sum of absolute terms so that a
cancelling sum has a bound at all); a result computed in double and stored as fp32 adds ``2^-24 |value|``.  A value stored as fp16 adds ``2^-11 |value|``, a split (hi, lo) pair ``2^-22 |value|``, and either
adds ``2^-25`` (half the spacing of fp16 subnormals: the last stored half may be one).  A loose ``n`` hides at most ``n * 2^-24`` of ``S``; the
defects the tests exist for (a dropped pixel, a wrong border tap, a lane counted twice) are of the order of one whole term of the sum --
tests/test_encoder_stream_oracle.py applies them to these very outputs and demands that ``ratio`` rejects each.

ReLU decisions.  A kernel decides ``ms*v + mt > 0`` with one fp32 FMA on fp32 copies of the float64 coefficients; where
``|ms*v + mt| < 2^-18 (|ms*v| + |mt|)`` it may decide the other way and move a whole gradient element.  ``deambiguate`` replaces such
elements in a generated input and ``mask_ambiguous`` counts them (the tests assert zero).  An element with ``ms*v`` and ``mt`` both exactly
zero is not ambiguous (0 > 0 is false in every precision) and is not counted.
"""
import math

import torch
import torch.nn.functional as F

U24 = 2.0 ** -24          # unit roundoff of fp32
F16_REL = 2.0 ** -11      # ... of fp16
SPLIT_REL = 2.0 ** -22    # a (hi, lo) pair of fp16
F16_SUB = 2.0 ** -25      # half the spacing of fp16 subnormals
DSUM_RTOL = 1e-12         # sums carried in double
MASK_MARGIN = 2.0 ** -18
INF = float("inf")

# ---- the cases of tests/test_encoder_stream_edges_gpu.py (shared with the defect tests, which run at the same shapes) ----------------------
CO1_CHANNELS = (8, 16, 128, 256, 512)
U1_CHANNELS = CO1_CHANNELS + (1024,)
CO1_SHAPES = ((1, 1, 1), (3, 1, 7), (3, 7, 1), (2, 2, 2), (3, 5, 7), (2, 3, 40), (2, 40, 3))
CO1_PAST_PROJ_CAP = (512, (33, 32, 32))   # 33792 pixels: above the projection's 2048, the weight gradient's and the statistics' 1024 workgroups
CO1_PAST_SHIFT_CAP = (8, (257, 64, 64))   # 1052672 pixels: above the shift pass's 4096 workgroups of 256
BN_CHANNELS = (8, 64, 2048)
PLUMB_SHAPES = ((1, 2, 2), (3, 2, 6), (3, 6, 2))
PLUMB_CHANNELS = ((8, 0), (8, 8), (24, 40))
POOL_CHANNELS = (8, 24)
SEED_SIZES = (1, 255, 257, 524289)


def bn_npix_cases(C):
    """pixel counts of the plain BatchNorm passes: 1 (no batch variance), 2 and 3 (a pair, a pair + an unpaired pixel), NPL + 1 (one pixel lane
    with two pixels), 105 (3x5x7), and 4097 where it exceeds the statistics' 1024-workgroup cap (C = 2048: one pixel lane, 4 pixels each)"""
    out = [1, 2, 3, npl(C) + 1, 105]
    if stats_grid(4097, C) == 1024 and -(-4097 // (npl(C) * 4)) > 1024:
        out.append(4097)
    return sorted(set(out))


# ---- launch geometry, as csrc/nastar_encoder_train_capi.hip documents it ---------------------------------------------------------------
def npl(C):
    """pixel lanes of a 256-thread workgroup: 256 / (C/8) eight-channel groups"""
    return 256 // (C // 8)


def stats_grid(npix, C):
    """workgroups of the two-stage statistics: >= 4 pixels per pixel lane, at most 1024"""
    return max(1, min(1024, -(-npix // (npl(C) * 4))))


def wgrad_grid(npix, C):
    """workgroups of the streamed weight gradient: 8 pixels per pixel lane, at most 1024"""
    return max(1, min(1024, -(-npix // (npl(C) * 8))))


def n_conv(C, fused):
    """fp32 roundings of one output of the closing convolution: 8 FMAs per tap and thread, log2(C/8) shuffle adds over the channel groups,
    9 adds in the shift pass (bias + nine taps); fused input relu(k2 z + k3): 2 more (multiply, add)"""
    return 8 + int(math.log2(C // 8)) + 9 + (2 if fused else 0)


def n_wgrad(npix, C, fused):
    """... of the streamed weight gradient: one FMA per pixel a lane walks (ceil(npix / (workgroups * NPL))), NPL adds over the pixel lanes
    in LDS, the workgroups' rows are added in double and stored as fp32 (1); fused input: 2 more"""
    return -(-npix // (wgrad_grid(npix, C) * npl(C))) + npl(C) + 1 + (2 if fused else 0)


N_U1 = 9      # the on-the-fly input gradient: nine FMAs (the weights times the power-of-two gscale are exact)
N_AFFINE = 3  # out = k2*v + k3 (2), + k1*u (1)
N_UPSUM = 4   # the 2x2 sum of the upsampling backward: four adds from zero
N_GRADADD = 3  # a*fa + b*fb: the factors are powers of two, one multiply-add; 3 covers an unfused multiply, multiply, add


# ---- operand view ------------------------------------------------------------------------------------------------------------------------
def seen(t, split):
    """float64 values a kernel reads from ``nhwc(t, split)``"""
    t = t.float()
    hi = t.to(torch.float16).float()
    return (hi + (t - hi).to(torch.float16).float() if split else hi).double()


def nhwc(t, split):
    """[B,C,H,W] -> the kernels' [B,H,W,C] fp16 (plain) or [B,H,W,(hi C | lo C)] (split)"""
    x = t.float().permute(0, 2, 3, 1).contiguous()
    hi = x.to(torch.float16)
    if split:
        return torch.cat((hi, (x - hi.float()).to(torch.float16)), dim=-1).contiguous()
    return hi.contiguous()


def from_nhwc(buf, C, split):
    """the float64 [B,C,H,W] value of a kernel's fp16 output buffer [B,H,W,C (x2)]"""
    o = buf.detach().cpu().double()
    return (o[..., :C] + (o[..., C:] if split else 0)).permute(0, 3, 1, 2).contiguous()


def store_bound(ref, split):
    return (SPLIT_REL if split else F16_REL) * ref.abs() + F16_SUB


def ratio(got, ref, bound):
    """largest |got - ref| / bound over the elements (0 where they are equal, inf where the bound is 0 and they are not, or where the
    result is not finite: an unwritten sentinel).  A result passes with ratio <= 1."""
    got, ref, bound = (torch.as_tensor(x, dtype=torch.float64).detach().cpu() for x in (got, ref, bound))
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = (got - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound.expand_as(err))
    r = torch.where(torch.isfinite(err), r, torch.full_like(err, INF))
    return float(r.max()) if r.numel() else 0.0


def _cvec(v):
    return torch.as_tensor(v, dtype=torch.float64).view(1, -1, 1, 1)


# ---- ReLU decisions ----------------------------------------------------------------------------------------------------------------------
def mask_ambiguous(v, ms, mt):
    """elements of v [B,C,H,W] whose ReLU decision ms*v + mt > 0 an fp32 FMA may take the other way"""
    a, b = _cvec(ms) * v, _cvec(mt)
    return (a + b).abs() < MASK_MARGIN * (a.abs() + b.abs())


def deambiguate(t, split, coef, rounds=8):
    """replace the elements of the generated tensor ``t`` (float32, before the fp16 view) whose decision is ambiguous under
    ``coef(seen(t)) -> (ms, mt)`` (the coefficients may depend on the tensor: batch statistics) by values a quarter further out;
    returns (t, seen(t))"""
    t = t.clone().float()
    for _ in range(rounds):
        v = seen(t, split)
        ms, mt = coef(v)
        bad = mask_ambiguous(v, ms, mt)
        if not bool(bad.any()):
            return t, v
        t = torch.where(bad, t + torch.where(t >= 0, 0.25, -0.25), t)
    raise AssertionError("ambiguous ReLU decisions remain")


# ---- the closing convolution Conv2d(C, 1, 3, padding=1) ----------------------------------------------------------------------------------
def co1_input(a, k2=None, k3=None):
    """(the layer's input, its absolute operand): ``a`` itself, or relu(k2*a + k3) formed in float64 with |k2||a| + |k3|"""
    if k2 is None:
        return a, a.abs()
    return torch.relu(_cvec(k2) * a + _cvec(k3)), _cvec(k2).abs() * a.abs() + _cvec(k3).abs()


def co1_forward(a, w, bias, n, k2=None, k3=None):
    """z [B,H,W] = conv2d(input, w [1,C,3,3], bias, padding=1) and its bound n * 2^-24 * conv2d(|input|, |w|, |bias|)"""
    x, xa = co1_input(a, k2, k3)
    b = None if bias is None else bias.double().view(1)
    z = F.conv2d(x, w.double(), b, padding=1)[:, 0]
    S = F.conv2d(xa, w.double().abs(), None if b is None else b.abs(), padding=1)[:, 0]
    return z, n * U24 * S


def co1_wgrad(d, a, n, k2=None, k3=None):
    """dW [1,C,3,3]: the float64 autograd formula of the convolution w.r.t. its weight (torch.nn.grad.conv2d_weight) for the upstream
    gradient d [B,H,W]; bound n * 2^-24 * S"""
    x, xa = co1_input(a, k2, k3)
    shape = (1, a.shape[1], 3, 3)
    dd = d.double()[:, None]
    dw = torch.nn.grad.conv2d_weight(x, shape, dd, padding=1)
    S = torch.nn.grad.conv2d_weight(xa, shape, dd.abs(), padding=1)
    return dw, n * U24 * S


def co1_u1(d, w, gscale, shape):
    """the "u1" tensor: gscale * (the float64 autograd formula of the convolution w.r.t. its input, torch.nn.grad.conv2d_input) [B,C,H,W],
    and its bound 9 * 2^-24 * S"""
    dd = d.double()[:, None]
    u = torch.nn.grad.conv2d_input(shape, w.double(), dd, padding=1) * gscale
    S = torch.nn.grad.conv2d_input(shape, w.double().abs(), dd.abs(), padding=1) * gscale
    return u, N_U1 * U24 * S


# ---- hidden-block BatchNorm2d (training mode) + ReLU -----------------------------------------------------------------------------------------
def bn_forward(z, gamma, beta, eps, momentum, rm, rv):
    """closed form of F.batch_norm(training=True): mean, invstd (biased variance), the folded scale / shift k2 = gamma invstd, k3 = beta - mean k2
    (a = relu(k2 z + k3)) and the running statistics after the update (unbiased variance; factor 1 for a single pixel, where torch refuses
    batch statistics).  tests/test_encoder_stream_oracle.py holds it against F.batch_norm itself."""
    gamma, beta = gamma.double(), beta.double()
    npix = z.numel() // z.shape[1]
    mean = z.mean(dim=(0, 2, 3))
    var = ((z - _cvec(mean)) ** 2).mean(dim=(0, 2, 3))
    invstd = 1.0 / torch.sqrt(var + eps)
    k2 = gamma * invstd
    k3 = beta - mean * k2
    fac = npix / (npix - 1.0) if npix > 1 else 1.0
    out = dict(mean=mean, var=var, invstd=invstd, k2=k2, k3=k3, npix=npix)
    if rm is not None:
        out["rm"] = (1 - momentum) * rm.double() + momentum * mean
        out["rv"] = (1 - momentum) * rv.double() + momentum * var * fac
    return out


def bn_forward_bounds(z, gamma, beta, eps, momentum, fwd):
    """bounds of the forward coefficients computed from double sums (sum z, sum z^2), each within 1e-12 of its sum of absolute terms"""
    gamma = gamma.double().abs()
    npix, mean, invstd = fwd["npix"], fwd["mean"].abs(), fwd["invstd"]
    e0 = DSUM_RTOL * z.abs().sum(dim=(0, 2, 3))
    e1 = DSUM_RTOL * (z * z).sum(dim=(0, 2, 3))
    d_mu = e0 / npix + 2.0 ** -52 * mean
    d_var = (e1 + 2 * mean * e0) / npix + 2.0 ** -51 * (z * z).mean(dim=(0, 2, 3))  # var = s1/n - mu^2: two double roundings of that size
    d_is = 0.5 * invstd ** 3 * d_var + 2.0 ** -51 * invstd
    fac = npix / (npix - 1.0) if npix > 1 else 1.0
    out = dict(sum0=e0, sum1=e1, mean=d_mu, invstd=d_is,
               k2=gamma * d_is + U24 * fwd["k2"].abs(),
               k3=gamma * (mean * d_is + invstd * d_mu) + U24 * fwd["k3"].abs())
    if "rm" in fwd:
        out["rm"] = momentum * d_mu + U24 * fwd["rm"].abs()
        out["rv"] = momentum * d_var * fac + U24 * fwd["rv"].abs()
    return out


def bn_relu_autograd(z, gamma, beta, eps, da):
    """F.batch_norm(training=True) + ReLU under float64 autograd for the upstream gradient ``da``: (a, dz, dgamma, dbeta)"""
    assert z.numel() // z.shape[1] > 1, "torch refuses batch statistics of one pixel: use the closed form"
    zz = z.clone().requires_grad_(True)
    g = gamma.double().clone().requires_grad_(True)
    b = beta.double().clone().requires_grad_(True)
    a = torch.relu(F.batch_norm(zz, None, None, g, b, True, 0.0, eps))
    a.backward(da)
    return a.detach(), zz.grad, g.grad, b.grad


def bn_backward(z, dy, gamma, fwd):
    """closed form of the BatchNorm backward for the masked gradient dy = da [a > 0]: the two sums, dgamma, dbeta, the coefficients of
    dz = c1 dy + c2 z + c3, and dz"""
    npix, mean, invstd = fwd["npix"], fwd["mean"], fwd["invstd"]
    sdy = dy.sum(dim=(0, 2, 3))
    sdyz = (dy * z).sum(dim=(0, 2, 3))
    sdyx = (sdyz - mean * sdy) * invstd
    k1 = gamma.double() * invstd
    m1, m2 = sdy / npix, sdyx / npix
    c1, c2, c3 = k1, -k1 * m2 * invstd, -k1 * m1 + k1 * m2 * mean * invstd
    dz = _cvec(c1) * dy + _cvec(c2) * z + _cvec(c3)
    return dict(sdy=sdy, sdyz=sdyz, dgamma=sdyx, dbeta=sdy, c1=c1, c2=c2, c3=c3, dz=dz)


def bn_backward_bounds(z, dy, e_dy, gamma, fwd, bwd):
    """bounds of the backward sums and coefficients; ``e_dy``: the bound of one element of dy (0 for a stored gradient, the u1 bound times
    the mask for the on-the-fly one).  The sums are double: 1e-12 of the absolute sum, plus the elements' own bounds."""
    npix, mean, invstd = fwd["npix"], fwd["mean"].abs(), fwd["invstd"]
    e0 = DSUM_RTOL * dy.abs().sum(dim=(0, 2, 3)) + e_dy.sum(dim=(0, 2, 3))
    e1 = DSUM_RTOL * (dy * z).abs().sum(dim=(0, 2, 3)) + (e_dy * z.abs()).sum(dim=(0, 2, 3))
    ex = (e1 + mean * e0) * invstd + 2.0 ** -51 * (bwd["sdyz"].abs() + mean * bwd["sdy"].abs()) * invstd  # sdyz - mean sdy cancels in double
    k1 = (gamma.double() * invstd).abs()
    m1, m2 = bwd["sdy"].abs() / npix, bwd["dgamma"].abs() / npix
    return dict(sdy=e0, sdyz=e1,
                dgamma=ex + U24 * bwd["dgamma"].abs(), dbeta=e0 + U24 * bwd["dbeta"].abs(),
                c1=U24 * bwd["c1"].abs(),
                c2=k1 * invstd * ex / npix + U24 * bwd["c2"].abs(),
                c3=k1 * (e0 / npix + ex / npix * mean * invstd) + U24 * (k1 * m1 + k1 * m2 * mean * invstd))


def affine_bound(c1, u_abs, c2, z, c3, split, n_u=0, coef_bounds=None, u=None):
    """bound of out = c1*u + c2*z + c3 stored as fp16 / split: (N_AFFINE + n_u) fp32 roundings of the absolute terms (``u_abs``: the masked
    |u|, or for an on-the-fly u its S with n_u = 9), the store, and -- against coefficients other than the kernel's own -- the
    coefficients' bounds times their factors"""
    S = _cvec(c1).abs() * u_abs + _cvec(c2).abs() * z.abs() + _cvec(c3).abs()
    ref = _cvec(c1) * (u if u is not None else 0) + _cvec(c2) * z + _cvec(c3)
    b = (N_AFFINE + n_u) * U24 * S + store_bound(ref, split)
    if coef_bounds is not None:
        b = b + _cvec(coef_bounds[0]) * (u.abs() if u is not None else 0) + _cvec(coef_bounds[1]) * z.abs() + _cvec(coef_bounds[2])
    return b


# ---- gradient scales -------------------------------------------------------------------------------------------------------------------------
def pow2_exponent(s):
    """e with s == 2^e exactly, else None"""
    s = float(s)
    if not (s > 0.0) or math.isinf(s):
        return None
    m, e = math.frexp(s)
    return e - 1 if m == 0.5 else None


def scale_window_ok(s, amax, lo, hi, amax_rel=0.0):
    """the documented choice S = 2^floor(log2(1024 / amax)) clamped to [2^lo, 2^hi], 1 for amax == 0: inside the clamp 512 < S amax <= 1024.
    The kernel divides (1 rounding) and takes log2f (1 ulp of an exponent up to |e| + 10) of an amax that went through up to 3 fp32
    roundings and may itself carry ``amax_rel``: the window is widened by exactly that"""
    e = pow2_exponent(s)
    if e is None or e < lo or e > hi:
        return False
    if amax == 0.0:
        return e == 0
    slack = amax_rel + 4 * U24 + 2.0 ** -23 * (abs(e) + 11) * math.log(2.0)
    p = float(s) * float(amax)
    if lo < e < hi:
        return 512.0 * (1 - slack) < p <= 1024.0 * (1 + slack)
    return p <= 1024.0 * (1 + slack) if e == hi else p > 512.0 * (1 - slack)


def grad_seed(d, S, split):
    """[npix, 32 (x2)] fp16: channel 0 = d * S as fp16 (its lo in split form), channels 1..31 zero"""
    x = d.float() * float(S)
    hi = x.to(torch.float16)
    out = torch.zeros((d.numel(), 64 if split else 32), dtype=torch.float16)
    out[:, 0] = hi
    if split:
        out[:, 32] = (x - hi.float()).to(torch.float16)
    return out


# ---- pooling / upsampling plumbing -----------------------------------------------------------------------------------------------------------
def maxpool_bwd(r, dp):
    """2x2 max-pool backward with the first-maximum tie rule (row-major window order), written out: no autograd"""
    B, C, H, W = r.shape
    win = r.view(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4)
    best = torch.zeros(win.shape[:-1], dtype=torch.long)
    top = win[..., 0].clone()
    for k in range(1, 4):
        better = win[..., k] > top
        best = torch.where(better, torch.full_like(best, k), best)
        top = torch.where(better, win[..., k], top)
    g = torch.zeros_like(win)
    g.scatter_(-1, best[..., None], dp[..., None].to(win.dtype))
    return g.view(B, C, H // 2, W // 2, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H, W)


def upcat(x, skip):
    """nearest x2 upsampling of x [B,C1,h,w], concatenated with skip [B,C2,2h,2w] (or nothing)"""
    up = x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    return up if skip is None else torch.cat((up, skip), dim=1)


def upcat_bwd(dcat, C1, split):
    """(d_x, its bound, d_skip): the 2x2 sums of the first C1 channels, the rest passed through"""
    B, C, H, W = dcat.shape
    blk = dcat[:, :C1].reshape(B, C1, H // 2, 2, W // 2, 2)
    dx = blk.sum(dim=(3, 5))
    S = blk.abs().sum(dim=(3, 5))
    return dx, N_UPSUM * U24 * S + store_bound(dx, split), dcat[:, C1:]


def grad_add(a, Sa, b, Sb, split):
    """two gradients of one tensor with scales Sa, Sb: (a So/Sa + b So/Sb, its bound, So = min(Sa, Sb))"""
    So = min(Sa, Sb)
    out = a * (So / Sa) + b * (So / Sb)
    S = a.abs() * (So / Sa) + b.abs() * (So / Sb)
    return out, N_GRADADD * U24 * S + store_bound(out, split), So
