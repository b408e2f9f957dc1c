"""Float64 restatement of the two fp16-MFMA layers of the encoder, as include/nastar.h defines them, with operands for which the device
result is determined to the BIT.  No GPU and nothing from the kernels' code: the operations are written from the header's formulas.

    nastar_conv3x3_f16 / nastar_conv3x3_img32_f16                                                                      conv_forward
        x   = cat(in (nearest x2 upsampled with UPSAMPLE), in2)                    NHWC, each given as a hi and a lo plane
        acc = conv3x3_pad1(x_hi, Wseg0) [+ conv3x3_pad1(x_lo, Wseg1) + conv3x3_pad1(x_hi, Wseg2)   with SPLIT]
        v   = clamp(relu?(acc * scale[n] + shift[n]), +-65504);  hi = fp16(v), lo = fp16(v - hi)
        FINAL|RAW: channel 0 of acc * scale + shift as fp32;  FINAL: final_mul / (1 + exp(-that))
    nastar_conv3x3_wgrad_f16                                                                                           conv_wgrad
        dw[co][ci][ky][kx] = (out_scale / gscale) * sum_{b,y,x} (dz_hi a_hi [+ dz_lo a_hi + dz_hi a_lo])[b, y, x, co; y+ky-1, x+kx-1, ci]

The kernels take their operands as plain arguments -- the activation planes, and for the convolution the weight pack itself -- so a test
may hand them three DIFFERENT weight segments and small integers: activations and dz in {-2..2}, weights in {-1, 0, 1}, scales +-2^k, integer
shifts, power-of-two gradient scales.  Every product is then an integer and, as long as ``precondition`` (the operation on absolute
operands) stays below 2^24 units of the result's finest fraction bit, so is every partial sum in ANY order: fp32 accumulation cannot round
and the expected device output is this oracle's, bit for bit.

``CONV_CASES`` / ``IMG32_CASES`` / ``WGRAD_CASES`` are the shapes both tests/test_mfma_conv_oracle.py (CPU) and
tests/test_mfma_conv_edges_gpu.py run; ``conv_geometry`` / ``wgrad_geometry`` restate the launch geometry of csrc/nastar_conv_flat.hip.h
and csrc/nastar_conv_wgrad.hip.h (for test ids, the recorded routes and the defects that need a chunk); ``CONV_DEFECTS`` / ``WGRAD_DEFECTS``
are faults a kernel of this design can have, applied to the oracle's own arithmetic: the CPU test demands that each changes the result at
every case it applies to, i.e. that the operands excite it.
"""
import collections
import zlib

import torch

EXACT_LIMIT = 2.0 ** 24   # integers below it are fp32 values, and so are their sums
F16_MAX = 65504.0
RELU, FINAL, UPSAMPLE, SPLIT, RAW = 1, 2, 4, 8, 16  # include/nastar.h: NASTAR_CONV_*

# ---- cases -----------------------------------------------------------------------------------------------------------------------------
# final: "" (fp16 tensor out), "raw" (FINAL|RAW) or "sig" (FINAL);  clamp: scales of +-2^6 and shifts up to +-66000, so that |v| passes 65504
ConvCase = collections.namedtuple("ConvCase", "B H W c1 c2 cout ups split relu final clamp")
WgradCase = collections.namedtuple("WgradCase", "B H W co ci co_real ci_real split out_scale gscale")


def _conv_rows(rows):
    out = []
    for i, (B, H, W, c1, c2, cout, ups, forms) in enumerate(rows):
        for split in forms:
            out.append(ConvCase(B, H, W, c1, c2, cout, ups, split, bool((i + split) & 1), "", False))
    return out


BOTH = (False, True)
FLAT_CASES = _conv_rows([
    (1, 1, 1, 32, 0, 32, False, BOTH),        # one pixel: centre tap only, 255 empty lanes
    (5, 1, 7, 32, 0, 64, False, BOTH),        # one-row images: every dy neighbour is another image
    (3, 9, 1, 32, 0, 32, False, BOTH),        # one-column images: every dx neighbour is another row
    (4, 8, 8, 64, 0, 64, False, BOTH),        # exactly one full tile
    (65, 2, 2, 64, 0, 96, False, BOTH),       # second tile of 4 pixels; NT = 32 with three channel blocks
    (3, 28, 28, 32, 0, 128, False, BOTH),     # 10 tiles (no multiple of 8) x 2 channel blocks: the XCD remap
    (2, 3, 126, 32, 0, 32, False, BOTH),      # widest flat row (halo 127), tile border mid-row
    (3, 6, 10, 32, 32, 64, True, BOTH),       # upsample + concat, half size 3 x 5 (odd)
    (7, 2, 2, 32, 0, 32, True, BOTH),         # upsample alone, half size 1 x 1
    (3, 2, 2, 512, 512, 64, True, (False,)),  # 32 slices
    (2, 4, 6, 96, 0, 32, False, (True,)),     # 3 x 3 slices
]) + [ConvCase(2, 5, 9, 32, 0, 32, False, split, relu, "", True) for split in BOTH for relu in BOTH   # the clamp, negative residuals
      ] + [ConvCase(9, 5, 5, 32, 0, 32, False, split, False, fin, False) for split in BOTH for fin in ("raw", "sig")]  # fp32 map, 225 pixels
WIDE_CASES = _conv_rows([
    (2, 1, 127, 32, 0, 32, False, BOTH),      # tile rows 1..3 empty
    (2, 5, 129, 32, 0, 32, False, BOTH),      # third tile one column wide, second tile row one row tall
    (1, 4, 128, 32, 0, 32, False, BOTH),      # exact tiles
    (2, 6, 130, 32, 32, 64, True, BOTH),      # upsample + concat at half width 65
]) + [ConvCase(1, 3, 131, 32, 0, 32, False, split, False, "raw", False) for split in BOTH]
CONV_CASES = FLAT_CASES + WIDE_CASES
IMG32_PAIRS = ((32, 64), (64, 128), (128, 256), (256, 128), (128, 64))  # include/nastar.h: nastar_conv3x3_img32_f16
IMG32_CASES = [ConvCase(3, 32, 32, cin, 0, cout, False, split, relu, "", False) for cin, cout in IMG32_PAIRS for split in BOTH for relu in BOTH]
FINAL_MULS = (1.0, 10.0)


def _wg(B, H, W, co, ci, crop=None, scales=(2.0, 4.0)):
    co_r, ci_r = crop if crop else (co - 3, ci - 5)
    return [WgradCase(B, H, W, co, ci, co_r, ci_r, split, scales[0], scales[1]) for split in BOTH]


WGRAD_CASES = (
    _wg(1, 1, 2, 32, 32)                      # smallest: G = 16 images per chunk, one present
    + _wg(17, 1, 2, 32, 32)                   # second chunk holds one image
    + _wg(11, 3, 3, 64, 32)                   # G = 8, limited by the 200 frame slots (pixels would allow 10); COB = 2
    + _wg(3, 2, 24, 32, 64)                   # 48 pixels: the pixel count admits two images, the slots one (G = 1); CIB = 2
    + _wg(2, 53, 2, 32, 32)                   # R = 1, NP = 2: one k-step with 14 zero rows; 106 chunks
    + _wg(1, 7, 13, 32, 32)                   # R = 7, 91 of 96 pixels in the sixth k-step
    + _wg(23, 8, 8, 64, 64)                   # 12 wavefronts; 23 chunks -> nsplit 5: one 4-block + a tail of 1
    + _wg(29, 8, 8, 32, 32)                   # nsplit 7: tail of 3; chunk sets of 5 and 4
    + _wg(9, 8, 8, 32, 32)                    # nsplit 2: chunk sets of 5 and 4, no 4-block at all
    + _wg(3, 5, 64, 32, 32)                   # last width of the narrow staging variant
    + _wg(2, 3, 65, 32, 32)                   # first ...
    + _wg(2, 2, 96, 32, 32)                   # ... and last width of the wide one
    + _wg(2, 2, 97, 32, 32)                   # ragged 49 + 48
    + _wg(1, 2, 194, 32, 64)                  # ragged 65 + 65 + 64: a middle segment with neighbours on both sides
    + _wg(1, 2, 192, 64, 32)                  # divisor segments of 96
    + _wg(2, 3, 128, 32, 32)                  # ... and of 64
    + _wg(2, 4, 4, 96, 160)                   # 15 channel tiles with COB = CIB = 1
    + _wg(2, 8, 8, 32, 256, crop=(1, 256))    # the closing layer's padded form
    + _wg(2, 8, 8, 64, 64, crop=(64, 64))     # nothing cropped
    + _wg(4, 6, 6, 32, 32, scales=(1.0, None))        # grad_scale_dev = NULL
    + _wg(4, 6, 6, 32, 32, scales=(2.0 ** -3, 2.0 ** 5))
)
WGRAD_NSPLIT = {(23, 8, 8, 64, 64): 5, (29, 8, 8, 32, 32): 7, (9, 8, 8, 32, 32): 2}  # what the list above counts on


def conv_id(c):
    return "B%d_%dx%d_c%d+%d_o%d%s_%s%s%s%s" % (c.B, c.H, c.W, c.c1, c.c2, c.cout, "_ups" if c.ups else "", "split" if c.split else "plain",
                                               "_relu" if c.relu else "", "_" + c.final if c.final else "", "_clamp" if c.clamp else "")


def wgrad_id(c):
    return "B%d_%dx%d_co%d_ci%d_r%dx%d_%s_s%g_g%s" % (c.B, c.H, c.W, c.co, c.ci, c.co_real, c.ci_real, "split" if c.split else "plain",
                                                      c.out_scale, "null" if c.gscale is None else "%g" % c.gscale)


def conv_flags(c):
    return ((RELU if c.relu else 0) | (UPSAMPLE if c.ups else 0) | (SPLIT if c.split else 0) | (FINAL if c.final else 0)
            | (RAW if c.final == "raw" else 0))


# ---- geometry mirrors (csrc/nastar_conv_flat.hip.h, csrc/nastar_conv_wgrad.hip.h and their host code) -------------------------------------
FLAT_MAXW, FLAT_TILE, WIDE_TW, WIDE_TH = 126, 256, 64, 4
WG_MAX_PIX, WG_MAX_SLOTS = 96, 200


def conv_geometry(c):
    wide = c.W > FLAT_MAXW
    ntiles = c.B * -(-c.H // WIDE_TH) * -(-c.W // WIDE_TW) if wide else -(-(c.B * c.H * c.W) // FLAT_TILE)
    nt = 32 if c.final else (64 if c.cout % 64 == 0 else 32)
    return dict(mode="wide" if wide else "flat", NT=nt, ntiles=ntiles, slices=(3 if c.split else 1) * (c.c1 + c.c2) // 32)


def wgrad_segment(W):
    """width of a chunk row: the image width up to 96; else the widest divisor in [64, 96]; else equal ragged segments"""
    if W <= WG_MAX_PIX:
        return W
    for d in range(WG_MAX_PIX, 63, -1):
        if W % d == 0:
            return d
    nseg = -(-W // WG_MAX_PIX)
    return -(-W // nseg)


def chunk_rows(H, W):
    """rows (row segments) per chunk, 0 = unsupported"""
    w = wgrad_segment(W)
    if w < 2 or w > WG_MAX_PIX or H <= 0:
        return 0
    if 64 % w == 0 and H % (64 // w) == 0:
        return 64 // w
    for r in range(WG_MAX_PIX // w, 0, -1):
        if H % r == 0:
            return r
    return 0


def chunk_images(H, W):
    """whole images per chunk: > 1 for images of at most 48 pixels, as many as fit 96 pixels and 200 framed slots"""
    if H * W > 48 or W > WG_MAX_PIX or chunk_rows(H, W) < H:
        return 1
    return max(1, min(WG_MAX_PIX // (H * W), WG_MAX_SLOTS // ((H + 2) * (W + 2))))


def wgrad_geometry(B, H, W, co, ci):
    seg = wgrad_segment(W)
    nseg = -(-W // seg)
    R, G = chunk_rows(H, W), chunk_images(H, W)
    assert R > 0
    NP = G * R * seg
    nchunk = -(-B // G) if G > 1 else (B * H // R) * nseg
    cob, cib = (2 if co % 64 == 0 else 1), (2 if ci % 64 == 0 else 1)
    tiles = (co // (32 * cob)) * (ci // (32 * cib))
    nsplit = max(1, min(256 // tiles, nchunk // 4))
    return dict(seg=seg, nseg=nseg, ragged=W % seg != 0, R=R, G=G, NP=NP, KS=-(-NP // 16), nchunk=nchunk, COB=cob, CIB=cib, tiles=tiles,
                nsplit=nsplit, staging="wide" if seg > 64 else "narrow")


def chunk_pixels(geo, B, H, W, ch):
    """bool [B,H,W]: the pixels of chunk ch"""
    m = torch.zeros((B, H, W), dtype=torch.bool)
    if geo["G"] > 1:
        m[ch * geo["G"]:(ch + 1) * geo["G"]] = True
        return m
    cr, s = divmod(ch, geo["nseg"])
    b, r = divmod(cr, H // geo["R"])
    m[b, r * geo["R"]:(r + 1) * geo["R"], s * geo["seg"]:(s + 1) * geo["seg"]] = True
    return m


# ---- the convolution ---------------------------------------------------------------------------------------------------------------------
def taps(x):
    """x [B,H,W,C] -> [B,H,W,9,C]: tap ky*3+kx of pixel (y, x) is x[b, y+ky-1, x+kx-1] or zero outside the image"""
    B, H, W, C = x.shape
    xp = x.new_zeros((B, H + 2, W + 2, C))
    xp[:, 1:H + 1, 1:W + 1] = x
    return torch.stack([xp[:, ky:ky + H, kx:kx + W] for ky in range(3) for kx in range(3)], dim=3)


def _wmat(w):
    """[cout, C, 3, 3] -> [9*C, cout], row = tap*C + c"""
    return w.permute(2, 3, 1, 0).reshape(-1, w.shape[0])


def _contract(t, w):
    B, H, W = t.shape[:3]
    return (t.reshape(B * H * W, -1) @ _wmat(w)).reshape(B, H, W, -1)


def upsample2(x):
    return x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


def assemble(a, b, ups, defect=None):
    """cat(in (upsampled), in2) along the channels"""
    if ups:
        if defect == "c":  # reads ((y + 1) / 2, (x + 1) / 2), zero beyond the half-size tensor
            B, h, w, C = a.shape
            ap = a.new_zeros((B, h + 1, w + 1, C))
            ap[:, :h, :w] = a
            a = upsample2(ap)[:, 1:2 * h + 1, 1:2 * w + 1]
        else:
            a = upsample2(a)
    if b is None:
        return a
    return torch.cat((b, a) if defect == "d" else (a, b), dim=-1)


def _defect_taps(t, x, defect):
    B, H, W, C = x.shape
    if defect == "a":  # right-hand neighbour at the last column = the next flat pixel (the next row's or the next image's first)
        t = t.clone()
        flat = torch.cat((x.reshape(-1, C), x.new_zeros((W + 2, C))))
        p = torch.arange(B * H * W).reshape(B, H, W)[:, :, W - 1]
        for ky in range(3):
            rows = [y for y in range(H) if 0 <= y + ky - 1 < H]
            t[:, rows, W - 1, ky * 3 + 2] = flat[p[:, rows] + (ky - 1) * W + 1]
    elif defect == "b":  # bottom neighbour at the last row = the next image's first row
        t = t.clone()
        xp = x.new_zeros((B + 1, W + 2, C))
        xp[:B - 1, 1:W + 1] = x[1:, 0]
        for kx in range(3):
            t[:, H - 1, :, 6 + kx] = xp[:B, kx:kx + W]
    elif defect == "g":  # taps mirrored in x
        t = t[:, :, :, [2, 1, 0, 5, 4, 3, 8, 7, 6]]
    return t


def conv_acc(ops, defect=None):
    """the accumulator [B,H,W,cout] float64"""
    c = ops["case"]
    xh = assemble(ops["in_hi"], ops["in2_hi"], c.ups, defect)
    th = _defect_taps(taps(xh), xh, defect)
    acc = _contract(th, ops["wseg"][0])
    if c.split:
        xl = assemble(ops["in_lo"], ops["in2_lo"], c.ups, defect)
        tl = _defect_taps(taps(xl), xl, defect)
        w1, w2 = (ops["wseg"][2], ops["wseg"][1]) if defect == "e" else (ops["wseg"][1], ops["wseg"][2])
        acc = acc + _contract(tl, w1) + _contract(th, w2)
        if defect == "f":
            acc = acc + _contract(tl, ops["wseg"][2])
    return acc


def f16(v):
    """float64 values that are fp32 values -> fp16, round to nearest even (one rounding: the step through fp32 is exact)"""
    f = v.float()
    assert torch.equal(f.double(), v), "not an fp32 value"
    return f.half()


def conv_value(ops, defect=None):
    """acc * scale + shift [B,H,W,cout] float64, after the optional ReLU and the clamp -- FINAL: channel 0 [B,H,W], neither applied"""
    c = ops["case"]
    v = conv_acc(ops, defect) * ops["scale"] + ops["shift"]
    if c.final:
        assert not c.relu, "the FINAL epilogue has no ReLU"
        return v[..., 0]
    if c.relu:
        v = v.clamp_min(0.0)
    return v.clamp(-F16_MAX, F16_MAX)


def conv_forward(ops, final_mul=1.0, defect=None):
    """dict: hi, lo (fp16 [B,H,W,cout], lo only when split) -- or f32 ([B,H,W] float64: raw channel 0, or its sigmoid * final_mul)"""
    c = ops["case"]
    v = conv_value(ops, defect)
    if c.final:
        if defect == "h":
            v = v.clone()
            v[:, :, -1] = 0
        return dict(z=v, f32=v if c.final == "raw" else final_mul / (1.0 + torch.exp(-v)))
    hi = f16(v)
    out = dict(v=v, hi=hi)
    if c.split:
        out["lo"] = f16(v - hi.double())
        if defect == "i":  # the ReLU after the rounding: a negative residual is lost
            out["lo"] = out["lo"].clamp_min(0)
    if defect == "h":
        for k in ("hi", "lo"):
            if k in out:
                out[k] = out[k].clone()
                out[k][:, :, -1] = 0
    return out


def conv_precondition(ops):
    """(largest |accumulator| any order of summation can reach, largest |acc * scale + shift| in units of its finest fraction bit)"""
    c = ops["case"]
    absops = dict(ops, case=c, wseg=[w.abs() for w in ops["wseg"]], **{k: (None if ops[k] is None else ops[k].abs())
                                                                      for k in ("in_hi", "in_lo", "in2_hi", "in2_lo")})
    acc = conv_acc(absops)
    unit = ops["scale"].abs().clamp(max=1.0)
    unit = torch.where(unit == 0, torch.ones_like(unit), unit)
    v = (acc * ops["scale"].abs() + ops["shift"].abs()) / unit
    return float(acc.max()), float(v.max())


def pack_weights(wsegs, split):
    """wpack[tap][v/8][n][v%8] fp16 with v = seg*(c1+c2) + c and tap = ky*3+kx (include/nastar.h); the plain form holds segment 0 only"""
    w = torch.cat(list(wsegs[:3] if split else wsegs[:1]), dim=1)  # [cout, V, 3, 3]
    cout, V = w.shape[:2]
    pack = torch.empty((9, V // 8, cout, 8), dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            pack[ky * 3 + kx] = w[:, :, ky, kx].reshape(cout, V // 8, 8).permute(1, 0, 2)
    return f16(pack)


def planes(hi, lo, split):
    """the kernel's activation argument: [.., C] fp16, or [.., hi(C) | lo(C)] when split"""
    if hi is None:
        return None
    return f16(torch.cat((hi, lo), dim=-1) if split else hi).contiguous()


def _seed(case, salt):
    return zlib.crc32(repr((tuple(case), salt)).encode())


def _ints(g, shape, lo, hi, density=1.0):
    t = torch.randint(lo, hi + 1, shape, generator=g).double()
    if density < 1.0:
        t = t * (torch.rand(shape, generator=g) < density)
    return t


def conv_operands(c):
    """seeded integer operands of a case.  Activations in {-2..2}, weights in {-1,0,1} (three independent segments), thinned where the
    channels are many; scales +-2^k, integer shifts; the last three output channels are padding (scale = shift = 0 over non-zero
    weights) unless the case is a FINAL one."""
    g = torch.Generator().manual_seed(_seed(c, "conv"))
    cin = c.c1 + c.c2
    dens = min(1.0, (64.0 / cin) ** 0.5)
    hw1 = (c.H // 2, c.W // 2) if c.ups else (c.H, c.W)
    ops = dict(case=c)
    ops["in_hi"] = _ints(g, (c.B,) + hw1 + (c.c1,), -2, 2, dens)
    ops["in_lo"] = _ints(g, (c.B,) + hw1 + (c.c1,), -2, 2, dens) if c.split else None
    ops["in2_hi"] = _ints(g, (c.B, c.H, c.W, c.c2), -2, 2, dens) if c.c2 else None
    ops["in2_lo"] = _ints(g, (c.B, c.H, c.W, c.c2), -2, 2, dens) if c.c2 and c.split else None
    ops["wseg"] = [_ints(g, (c.cout, cin, 3, 3), -1, 1, dens) for _ in range(3)]
    sign = _ints(g, (c.cout,), 0, 1) * 2 - 1
    if c.clamp:
        scale, shift = sign * 64.0, _ints(g, (c.cout,), -66000, 66000)
        shift[:4] = torch.tensor([66000.0, -66000.0, 65001.0, -65001.0], dtype=torch.float64)  # both clamps, and values just inside them
    elif c.final:
        scale, shift = sign * 0.25, _ints(g, (c.cout,), -2, 2)
    else:
        scale, shift = sign * 2.0 ** _ints(g, (c.cout,), -1, 3), _ints(g, (c.cout,), -5000, 5000)
    if not c.final:
        scale[-3:] = 0
        shift[-3:] = 0
    ops["scale"], ops["shift"] = scale, shift
    return ops


# ---- defects of the convolution: letter -> (what, applies(case)) ------------------------------------------------------------------------
CONV_DEFECTS = {
    "a": ("the right-hand neighbour at the last column is the next flat pixel (row wrap)", lambda c: c.W <= FLAT_MAXW and c.B * c.H * c.W > 1),
    "b": ("the bottom neighbour at the last row is the next image's first row", lambda c: c.B > 1),
    "c": ("upsampling reads ((y+1)/2, (x+1)/2)", lambda c: c.ups),
    "d": ("concatenation order exchanged", lambda c: c.c2 > 0),
    "e": ("segments 1 and 2 exchanged", lambda c: c.split),
    "f": ("an x_lo * Wseg2 term added", lambda c: c.split),
    "g": ("taps mirrored in x", lambda c: c.W > 1),
    "h": ("the last column of a wide image is zero in the output", lambda c: c.W > FLAT_MAXW),
    "i": ("ReLU applied after the fp16 rounding of a negative residual", lambda c: c.split and c.clamp),
}


def conv_differs(a, b):
    return any(not torch.equal(a[k], b[k]) for k in ("hi", "lo", "f32") if k in a)


# ---- the weight gradient -----------------------------------------------------------------------------------------------------------------
def _outer(dz, t):
    """dz [B,H,W,co], t [B,H,W,9,ci] -> [co, ci, 3, 3]"""
    co, ci = dz.shape[-1], t.shape[-1]
    return (dz.reshape(-1, co).t() @ t.reshape(-1, 9 * ci)).reshape(co, 3, 3, ci).permute(0, 3, 1, 2)


def wgrad_sum(ops, defect=None, absolute=False):
    """sum over pixels of the (three) products, uncropped [co, ci, 3, 3] float64"""
    c = ops["case"]
    f = (lambda t: t.abs()) if absolute else (lambda t: t)
    geo = wgrad_geometry(c.B, c.H, c.W, c.co, c.ci)
    keep = torch.ones((c.B, c.H, c.W), dtype=torch.bool)
    if defect == "j":    # the last column of a ragged segment dropped
        keep[:, :, c.W - 1] = False
    elif defect == "l":  # the images of a partial last chunk dropped
        keep[(c.B // geo["G"]) * geo["G"]:] = False
    elif defect == "o":  # the splits beyond the last multiple of four left out of the sum (chunk ch belongs to split ch % nsplit)
        for ch in range(geo["nchunk"]):
            if ch % geo["nsplit"] >= geo["nsplit"] // 4 * 4:
                keep &= ~chunk_pixels(geo, c.B, c.H, c.W, ch)
    k = keep.unsqueeze(-1)
    dzh, dzl = f(ops["dz_hi"]) * k, (f(ops["dz_lo"]) * k if c.split else None)
    th = taps(f(ops["a_hi"]))
    tl = taps(f(ops["a_lo"])) if c.split else None
    if defect == "k":    # a segment's frame column is zero where the neighbouring segment holds a pixel
        x = torch.arange(c.W)
        first, last = (x % geo["seg"] == 0) & (x > 0), (x % geo["seg"] == geo["seg"] - 1) & (x < c.W - 1)
        th, tl = th.clone(), (tl.clone() if c.split else None)
        for t in (th, tl) if c.split else (th,):
            for ky in range(3):
                t[:, :, first, ky * 3 + 0] = 0
                t[:, :, last, ky * 3 + 2] = 0
    dw = _outer(dzh, th)
    if c.split:
        if defect != "m":  # the dz_lo * a_hi term dropped
            dw = dw + _outer(dzl, th)
        dw = dw + _outer(dzh, tl)
    if defect == "n":    # the dz rows of the partial last k-step not zero: the pixel after a chunk meets the chunk's last pixel's neighbours
        npix = c.B * c.H * c.W
        last = torch.arange(geo["NP"] - 1, npix - 1, geo["NP"])
        pick = lambda t: t.reshape(npix, *t.shape[3:])
        dw = dw + _outer(pick(ops["dz_hi"])[last + 1].reshape(1, 1, -1, c.co), pick(th)[last].reshape(1, 1, -1, 9, c.ci))
    return dw


def conv_wgrad(ops, defect=None):
    """dw [co_real, ci_real, 3, 3] float64 (defect "p", the crop ignored: the whole padded tensor)"""
    c = ops["case"]
    dw = wgrad_sum(ops, defect) * (c.out_scale / (c.gscale if c.gscale is not None else 1.0))
    return dw if defect == "p" else dw[:c.co_real, :c.ci_real].contiguous()


def wgrad_precondition(ops):
    """largest sum of |dz| |a| over the (three) terms"""
    return float(wgrad_sum(ops, absolute=True).max())


def wgrad_operands(c):
    """seeded integer operands in {-2..2}, every padded channel included (a crop that is ignored shows)"""
    g = torch.Generator().manual_seed(_seed(c[:5], "wgrad"))
    ops = dict(case=c)
    for name, ch in (("dz_hi", c.co), ("dz_lo", c.co), ("a_hi", c.ci), ("a_lo", c.ci)):
        ops[name] = _ints(g, (c.B, c.H, c.W, ch), -2, 2)
    return ops


def _geo(c):
    return wgrad_geometry(c.B, c.H, c.W, c.co, c.ci)


WGRAD_DEFECTS = {
    "j": ("the last column of a ragged segment dropped", lambda c: _geo(c)["ragged"]),
    "k": ("a segment's frame column zero where the neighbouring segment holds a pixel", lambda c: _geo(c)["nseg"] > 1),
    "l": ("the images of a partial last chunk dropped", lambda c: _geo(c)["G"] > 1 and c.B % _geo(c)["G"] != 0),
    "m": ("the dz_lo * a_hi term dropped", lambda c: c.split),
    "n": ("dz rows of the partial last k-step not zero", lambda c: _geo(c)["NP"] % 16 != 0 and _geo(c)["nchunk"] > 1 and _geo(c)["nseg"] == 1),
    "o": ("the splits beyond the last multiple of four left out of the sum", lambda c: _geo(c)["nsplit"] % 4 != 0),
    "p": ("padded channels written (crop ignored)", lambda c: c.co_real < c.co or c.ci_real < c.ci),
}


def wgrad_differs(clean, bad):
    return clean.shape != bad.shape or not torch.equal(clean, bad)
