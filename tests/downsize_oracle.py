"""Float64 restatement of what nastar_encoder_cnn_downsize_forward promises (include/nastar.h), level by level.  No GPU, nothing from
the kernels: the operations are written as the header and the reference's modules define them (planner/encoder.py:81-97 CNNDownSize,
:32-34 sigmoid * const, astar.py:171-177 input assembly):

    x    = cat(image, F.interpolate(start + goal, size=(H, W), mode="nearest")), NHWC, zero padded to CP channels          prep
    x    = maxpool2x2(relu(conv3x3_pad1(x) * scale + shift))                           once per hidden block               hidden
    cost = final_mul * sigmoid(conv3x3_pad1(x) * scale + shift)[..., 0]                                                    final

Tensors are NHWC float64; weights are [9][CINp][COUTp] with tap = ky*3 + kx, scale / shift [COUTp], as the header lays them out.

``levels`` is the workspace layout the header documents (prep tensor first, then one pooled tensor per hidden block, in order, nothing
between them); tests/test_encoder_downsize_edges_gpu.py reads every level back from the workspace with it.

``exact_operands`` draws integer-valued operands for which every fp32 operation of the forward pass is exact in any summation order,
so that every level the device stores must have the oracle's bits; ``exactness`` is the precondition that says so (see there).
"""
import math

import torch
import torch.nn.functional as F

KINDS = {"m": (1, False), "m+": (1, True), "rgb": (3, False), "rgb+": (3, True)}  # encoder_input -> (image channels, plus)
HIDDEN = (32, 64, 128, 256)  # output channels of the hidden blocks (reference encoder.py:62)
FINAL_COUTP = 32             # the last block's single channel, padded
EXACT_LIMIT = 2.0 ** 24      # integers below it are fp32 values, and so are their sums

# kind, depth, H, W, B: the smallest shapes that make each path of the 2-row x 16-column output tile partial (the GPU file says what each reaches)
CASES = (
    ("m", 1, 2, 2, 3),
    ("m+", 1, 6, 34, 2),
    ("rgb", 2, 8, 72, 2),
    ("rgb+", 3, 24, 40, 37),
    ("m+", 4, 16, 16, 2),
    ("m+", 4, 32, 48, 1),
    ("rgb+", 3, 96, 96, 2),
)
FINAL_MULS = (1.0, 10.0)
# start / goal upsampling: the cases with a start + goal channel (but the largest) at h x w = H>>depth x W>>depth and = H x W, and one
# ratio that is no integer, 88/26 x 112/62 (H, W, h, w), at depth 1, C = 1, B = 1
UPSAMPLE_CASES = tuple(c for c in CASES if KINDS[c[0]][1] and c[2] * c[3] <= 32 * 48)
NONINTEGER_RATIO = (88, 112, 26, 62)
NONINTEGER_PATTERNS = ("one-hot", "dense")


def cin_pad(cin):
    """input channels of the first block as the workspace holds them: 2 or 4"""
    assert 1 <= cin <= 4
    return 2 if cin <= 2 else 4


def case_id(case):
    kind, depth, H, W, B = case
    return "%s-d%d-%dx%d-B%d" % (kind, depth, H, W, B)


# ---- nearest-neighbour source indices ------------------------------------------------------------------------------------------------------
def nearest_source_index(n_in, n_out):
    """Source index of every output position under F.interpolate(mode="nearest") on an fp32 tensor, read off torch itself:
    min(int(floorf(y * (float(n_in) / n_out))), n_in - 1).  The ramp must be fp32, the type the reference's modules and this package's
    training path run in: for a float64 tensor torch's CPU kernel takes the ratio in double, which names other cells for 346 of the
    (n_in, n_out) pairs with even n_out < 260."""
    assert n_in < 1 << 24
    ramp = torch.arange(n_in, dtype=torch.float32).view(1, 1, n_in, 1)
    return F.interpolate(ramp, size=(n_out, 1), mode="nearest").view(n_out).long()


def integer_source_index(n_in, n_out):
    """(y * n_in) // n_out: equal to the above for integer ratios, not in general"""
    return (torch.arange(n_out) * n_in) // n_out


def index_differences(n_in, n_out):
    """output positions at which the two formulas name different source positions"""
    return (nearest_source_index(n_in, n_out) != integer_source_index(n_in, n_out)).nonzero().flatten().tolist()


# ---- the three operations ------------------------------------------------------------------------------------------------------------------
def prep(image, start, goal, plus, CP):
    """image [B,C,H,W], start / goal [B,h,w] (ignored unless plus) -> [B,H,W,CP] float64"""
    image = image.double()
    B, C, H, W = image.shape
    x = image
    if plus:
        sg = start.double() + goal.double()  # F.interpolate(sg.float(), size=(H, W), mode="nearest"), kept in float64
        ys, xs = nearest_source_index(sg.shape[-2], H), nearest_source_index(sg.shape[-1], W)
        x = torch.cat((x, sg[:, ys][:, :, xs].unsqueeze(1)), dim=1)
    assert x.shape[1] <= CP
    out = torch.zeros((B, H, W, CP), dtype=torch.float64)
    out[..., :x.shape[1]] = x.permute(0, 2, 3, 1)
    return out


def conv3x3(x, w):
    """x [B,H,W,CIN], w [9][CIN][COUT] (tap = ky*3 + kx), zero padding 1 -> [B,H,W,COUT]"""
    B, H, W, cin = x.shape
    assert w.shape[:2] == (9, cin)
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    out = torch.zeros((B, H, W, w.shape[2]), dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            out += xp[:, ky:ky + H, kx:kx + W, :] @ w[ky * 3 + kx]
    return out


def hidden(x, w, scale, shift):
    B, H, W, _ = x.shape
    assert H % 2 == 0 and W % 2 == 0
    y = torch.relu(conv3x3(x, w) * scale + shift)
    return y.view(B, H // 2, 2, W // 2, 2, -1).amax(dim=(2, 4))


def final_preact(x, w, scale, shift):
    return (conv3x3(x, w) * scale + shift)[..., 0]


def final(x, w, scale, shift, mul):
    return mul * torch.sigmoid(final_preact(x, w, scale, shift))


def chain(image, start, goal, plus, wts, scale, shift, mul):
    """-> ([prep tensor, pooled tensor of every hidden block], pre-activation of the cost map [B,Ho,Wo], cost map)"""
    depth = len(wts) - 1
    wts, scale, shift = ([t.double() for t in ts] for ts in (wts, scale, shift))
    x = prep(image, start, goal, plus, wts[0].shape[1])
    lv = [x]
    for l in range(depth):
        x = hidden(x, wts[l], scale[l], shift[l])
        lv.append(x)
    z = final_preact(x, wts[depth], scale[depth], shift[depth])
    return lv, z, mul * torch.sigmoid(z)


# ---- the workspace ---------------------------------------------------------------------------------------------------------------------------
def levels(B, Cin, H, W, depth):
    """-> ([(offset in floats, shape)] for the prep tensor and every pooled tensor, workspace bytes): the sum that
    nastar_encoder_downsize_workspace_bytes is documented to return, term by term"""
    assert B > 0 and 1 <= Cin <= 4 and 1 <= depth <= 4 and H % (1 << depth) == 0 and W % (1 << depth) == 0
    out, off = [], 0
    shapes = [(B, H, W, cin_pad(Cin))] + [(B, H >> (l + 1), W >> (l + 1), 32 << l) for l in range(depth)]
    for shp in shapes:
        out.append((off, shp))
        off += math.prod(shp)
    return out, off * 4


# ---- operands that make fp32 exact -----------------------------------------------------------------------------------------------------------
def one_hot(B, h, w, g):
    t = torch.zeros((B, h * w), dtype=torch.float64)
    t[torch.arange(B), torch.randint(0, h * w, (B,), generator=g)] = 1.0
    return t.view(B, h, w)


def sparse_weights(cin_p, cout, nnz, g):
    """[9][cin_p][cout] in {-1, 0, +1}: every output channel has min(nnz, 9 cin_p) non-zero (tap, cin) slots, drawn so that every slot is
    taken by some channel when cout * nnz >= 9 cin_p (a rotation through a random permutation of the slots, then random signs)"""
    slots = 9 * cin_p
    nnz = min(nnz, slots)
    perm = torch.randperm(slots, generator=g)
    w = torch.zeros((slots, cout), dtype=torch.float64)
    for n in range(cout):
        idx = perm[(torch.arange(nnz) + n * nnz) % slots]
        w[idx, n] = (torch.randint(0, 2, (nnz,), generator=g) * 2 - 1).double()
    return w.view(9, cin_p, cout)


def _pow2(values, n, g):
    return torch.tensor(values, dtype=torch.float64)[torch.randint(0, len(values), (n,), generator=g)]


def exact_operands(kind, depth, H, W, B, seed=0, hw=None, draws=8):
    """Operands of one forward call, all float64 tensors holding fp32 values: image in {-2..2}, one-hot start / goal [B,h,w] (hw, default
    H>>depth x W>>depth), weights in {-1,0,+1} (16 per hidden output channel; the last block's channel 0 dense, its 31 padded channels
    given weights, scales and shifts too: they must not reach the cost map), scales +-2^k, integer shifts.

    A hidden block's shift is minus the (integer) 0.9 quantile of its channel's scaled convolution, which keeps a tenth of the
    pre-pool activations; the last block's scale brings the cost map's pre-activation to a spread of a few units and its shift centres
    it.  The last block is drawn up to `draws` times until `exactness` holds."""
    C, plus = KINDS[kind]
    cp = cin_pad(C + plus)
    g = torch.Generator().manual_seed(1000 * seed + 7 * H + W + 31 * depth + B)
    image = torch.randint(-2, 3, (B, C, H, W), generator=g).double()
    h, w = hw if hw is not None else (H >> depth, W >> depth)
    start, goal = (one_hot(B, h, w, g), one_hot(B, h, w, g)) if plus else (None, None)
    ops = dict(kind=kind, C=C, plus=plus, depth=depth, B=B, H=H, W=W, h=h, w=w, image=image, start=start, goal=goal, wts=[], scale=[], shift=[])
    x = prep(image, start, goal, plus, cp)
    for l in range(depth):
        cin_p, cout = x.shape[-1], HIDDEN[l]
        wt = sparse_weights(cin_p, cout, 16, g)
        sc = _pow2((0.5, 1.0, -1.0, 2.0), cout, g)
        pre = (conv3x3(x, wt) * sc).reshape(-1, cout)
        sh = -torch.ceil(torch.quantile(pre, 0.9, dim=0, interpolation="lower"))
        ops["wts"].append(wt); ops["scale"].append(sc); ops["shift"].append(sh)
        x = hidden(x, wt, sc, sh)
    cin_p = x.shape[-1]
    for _ in range(draws):
        wt = sparse_weights(cin_p, FINAL_COUTP, 16, g)
        wt[:, :, 0] = (torch.randint(0, 2, (9, cin_p), generator=g) * 2 - 1).double()
        conv0 = conv3x3(x, wt)[..., 0]
        spread = float(conv0.std()) if conv0.numel() > 1 else 0.0
        k = max(0, math.ceil(math.log2(spread / 2.0))) if spread > 2.0 else 0
        sc = _pow2((0.5, 1.0, -1.0, 2.0), FINAL_COUTP, g)
        sh = torch.randint(-3, 4, (FINAL_COUTP,), generator=g).double()
        sc[0] = 2.0 ** -k
        sh[0] = -torch.round((conv0 * sc[0]).mean())
        cand = dict(ops, wts=ops["wts"] + [wt], scale=ops["scale"] + [sc], shift=ops["shift"] + [sh])
        if max(exactness(cand)) < EXACT_LIMIT:
            return cand
    raise AssertionError("no exact draw of the last block for %s" % (case_id((kind, depth, H, W, B)),))


def exactness(ops):
    """Per block, max over its stored outputs of  (conv(|x|, |w|) * |scale| + |shift|) / unit,  x the block's input in the float64 chain.

    `unit` is a power of two that divides every value the block can produce: the prep tensor holds integers (unit 1); a block whose
    input has unit u, whose scales are +-2^k and whose shifts are integers produces multiples of min(1, u * min|scale|).  Every partial
    sum of the convolution, in any order, is a multiple of u no larger than conv(|x|, |w|); its scaled and shifted value is a multiple
    of the block's unit no larger than the expression above.  Below 2^24 units all of them are fp32 values, so no fp32 addition,
    multiplication or fused multiply-add on the way rounds, and ReLU and max only select.  Only channel 0 of the last block is stored."""
    for ts in (ops["wts"], ops["scale"], ops["shift"]):
        assert all(torch.equal(t.float().double(), t) for t in ts), "operands must be fp32 values"
    assert all(bool((torch.log2(s.abs()) % 1 == 0).all()) for s in ops["scale"]), "scales must be powers of two"
    assert all(bool((s % 1 == 0).all()) for s in ops["shift"]), "shifts must be integers"
    depth = ops["depth"]
    lv, _, _ = chain(ops["image"], ops["start"], ops["goal"], ops["plus"], ops["wts"], ops["scale"], ops["shift"], 1.0)
    assert bool((lv[0] % 1 == 0).all()), "the prep tensor must hold integers"
    unit, out = 1.0, []
    for l in range(depth + 1):
        sc, sh = ops["scale"][l].abs(), ops["shift"][l].abs()
        if l == depth:
            sc, sh = sc[:1], sh[:1]
        unit = min(1.0, unit * float(sc.min()))
        mag = conv3x3(lv[l].abs(), ops["wts"][l].abs())[..., :sc.numel()] * sc + sh
        out.append(float(mag.max()) / unit)
    return out


def upsample_sizes(case):
    kind, depth, H, W, B = case
    return ((H >> depth, W >> depth), (H, W))


def noninteger_operands(pattern):
    """Exact operands at NONINTEGER_RATIO whose start / goal maps tell F.interpolate from (y * h) // H: "one-hot" puts the start on the
    source cell F.interpolate shows at the first output row and column where the two formulas differ and the goal on the cell the
    integer formula shows there; "dense" is a start map of random {0, 1, 2} with an empty goal map."""
    H, W, h, w = NONINTEGER_RATIO
    ops = exact_operands("m+", 1, H, W, 1, hw=(h, w))
    y, x = index_differences(h, H)[0], index_differences(w, W)[0]
    start, goal = torch.zeros((1, h, w), dtype=torch.float64), torch.zeros((1, h, w), dtype=torch.float64)
    if pattern == "one-hot":
        start[0, nearest_source_index(h, H)[y], nearest_source_index(w, W)[x]] = 1.0
        goal[0, integer_source_index(h, H)[y], integer_source_index(w, W)[x]] = 1.0
    else:
        assert pattern == "dense"
        start = torch.randint(0, 3, (1, h, w), generator=torch.Generator().manual_seed(2)).double()
    return dict(ops, start=start, goal=goal)


def all_exact_operands():
    """(name, operands) of every launch tests/test_encoder_downsize_edges_gpu.py holds to the oracle's bits"""
    for case in CASES:
        yield case_id(case), exact_operands(*case)
    for case in UPSAMPLE_CASES:
        for hw in upsample_sizes(case):
            yield case_id(case) + "-from-%dx%d" % hw, exact_operands(*case, hw=hw)
    for pattern in NONINTEGER_PATTERNS:
        yield "noninteger-" + pattern, noninteger_operands(pattern)
