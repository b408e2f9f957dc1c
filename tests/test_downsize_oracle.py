"""tests/downsize_oracle.py against the torch CNNDownSize module in float64, its exactness precondition at every case the GPU file
(tests/test_encoder_downsize_edges_gpu.py) uses, and the nearest-neighbour index table that tells F.interpolate from (y * h) // H.
Runs without a GPU."""
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import downsize_oracle as O


def dyadic_module(kind, depth, const, seed):
    """A random CNNDownSize whose eval-mode BatchNorm folds into fp32 scale / shift without rounding, so that fold_bn (which returns
    fp32) loses nothing and the comparison below can ask for 1e-12: eps = 2^-10, running_var = 4^k - eps (k = -1, 0, 1: var + eps is an
    exact square), BatchNorm weight / bias / running_mean and the conv bias multiples of 1/16.  The conv weights are random fp32 values."""
    from neural_astar.planner.encoder import CNNDownSize
    g = torch.Generator().manual_seed(seed)
    C, plus = O.KINDS[kind]
    cnn = CNNDownSize(C + plus, depth, const)
    sixteenths = lambda n, lo, hi: torch.randint(lo, hi, (n,), generator=g).float() / 16
    with torch.no_grad():
        for m in cnn.model:
            if isinstance(m, nn.Conv2d):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / (9 * m.in_channels)) ** 0.5)
                m.bias.copy_(sixteenths(m.out_channels, -8, 9))
            if isinstance(m, nn.BatchNorm2d):
                n = m.num_features
                m.eps = 2.0 ** -10
                m.running_var.copy_(4.0 ** torch.randint(-1, 2, (n,), generator=g).float() - m.eps)
                m.running_mean.copy_(sixteenths(n, -8, 9))
                m.weight.copy_(sixteenths(n, 8, 25))
                m.bias.copy_(sixteenths(n, -4, 5))
    return cnn.eval()


def folded(cnn):
    """(wts, scale, shift) of a CNNDownSize as the C entry takes them, by the package's own fold_bn and pack_conv_weight_f32"""
    from neural_astar.encoder_hip import fold_bn, pack_conv_weight_f32
    layers = list(cnn.model)
    convs = [i for i, m in enumerate(layers) if isinstance(m, nn.Conv2d)]
    wts, scale, shift = [], [], []
    for k, i in enumerate(convs):
        conv, last = layers[i], k == len(convs) - 1
        cin_p = O.cin_pad(conv.in_channels) if k == 0 else conv.in_channels
        cout_p = O.FINAL_COUTP if last else conv.out_channels
        wts.append(pack_conv_weight_f32(conv.weight, cin_p, cout_p))
        sc, sh = fold_bn(conv, layers[i + 1], cout_p)
        scale.append(sc); shift.append(sh)
    return wts, scale, shift


@pytest.mark.parametrize("depth", [1, 2, 3, 4])
@pytest.mark.parametrize("kind", list(O.KINDS))
def test_oracle_chain_is_the_float64_module(kind, depth):
    C, plus = O.KINDS[kind]
    const = None if depth % 2 else 3.0
    cnn = dyadic_module(kind, depth, const, seed=11 * depth + len(kind))
    B, H, W = 2, 16, 48
    g = torch.Generator().manual_seed(depth)
    image = torch.rand((B, C, H, W), generator=g).double()
    h, w = H >> depth, W >> depth
    start, goal = O.one_hot(B, h, w, g), O.one_hot(B, h, w, g)
    wts, scale, shift = folded(cnn)
    mul = 1.0 if const is None else const
    lv, z, cost = O.chain(image, start, goal, plus, wts, scale, shift, mul)

    c64 = cnn.double()
    x = image
    if plus:
        x = torch.cat((x, F.interpolate((start + goal).unsqueeze(1), size=(H, W), mode="nearest")), dim=1)
    with torch.no_grad():
        want = c64(x)[:, 0]
        # every pooled level: the module cut after each MaxPool2d
        acts, t = [], x
        for m in c64.model:
            t = m(t)
            if isinstance(m, nn.MaxPool2d):
                acts.append(t.permute(0, 2, 3, 1))
    assert cost.shape == want.shape == (B, h, w)
    assert float(want.std()) > 1e-3
    assert float((cost - want).abs().max()) <= 1e-12
    assert len(acts) == depth == len(lv) - 1
    for l, a in enumerate(acts):
        assert lv[l + 1].shape == a.shape and float(a.abs().max()) > 0
        assert float((lv[l + 1] - a).abs().max()) <= 1e-12, l
    assert torch.equal(lv[0][..., :C + plus], x.permute(0, 2, 3, 1)) and not bool(lv[0][..., C + plus:].any())


def test_levels_follow_the_workspace_formula():
    lv, nbytes = O.levels(5, 4, 96, 96, 3)
    assert lv == [(0, (5, 96, 96, 4)), (184320, (5, 48, 48, 32)), (552960, (5, 24, 24, 64)), (737280, (5, 12, 12, 128))]
    assert nbytes == 4 * (737280 + 5 * 12 * 12 * 128)
    lv, nbytes = O.levels(3, 1, 2, 2, 1)
    assert lv == [(0, (3, 2, 2, 2)), (24, (3, 1, 1, 32))] and nbytes == 4 * (24 + 96)
    from neural_astar import _native
    lib = _native.load()
    for kind, depth, H, W, B in O.CASES:
        C, plus = O.KINDS[kind]
        assert O.levels(B, C + plus, H, W, depth)[1] == int(lib.nastar_encoder_downsize_workspace_bytes(B, C + plus, H, W, depth))


def test_every_launch_held_to_bits_meets_the_precondition():
    names = []
    for name, ops in O.all_exact_operands():
        ex = O.exactness(ops)
        print(name, "log2 of the largest magnitude in units, per block:", ["%.1f" % math.log2(e) for e in ex])
        assert max(ex) < O.EXACT_LIMIT, name
        names.append(name)
    assert len(names) == len(set(names)) == len(O.CASES) + 2 * len(O.UPSAMPLE_CASES) + len(O.NONINTEGER_PATTERNS)
    assert len(O.UPSAMPLE_CASES) == 4


@pytest.mark.parametrize("case", O.CASES, ids=O.case_id)
def test_exact_operands_keep_fp32_exact_and_every_level_alive(case):
    """the precondition of the bit-exact GPU test, and that its operands exercise the network: every level has non-zero and zero
    activations, every (tap, cin) slot of every hidden block carries a weight, the cost map is not saturated"""
    ops = O.exact_operands(*case)
    ex = O.exactness(ops)
    assert max(ex) < O.EXACT_LIMIT
    lv, z, cost = O.chain(ops["image"], ops["start"], ops["goal"], ops["plus"], ops["wts"], ops["scale"], ops["shift"], 1.0)
    for t in lv + [z]:
        assert torch.equal(t.float().double(), t)
    for l, t in enumerate(lv[1:]):
        density = float((t != 0).double().mean())
        assert 0.05 < density < 0.95, (l, density)
    for wt in ops["wts"]:
        assert bool((wt != 0).any(dim=2).all()), "a (tap, cin) slot no output channel reads"
    assert bool((ops["wts"][-1][:, :, 0] != 0).all())
    assert bool(ops["wts"][-1][:, :, 1:].any()) and bool(ops["scale"][-1][1:].all()), "the padded channels of the last block must carry something"
    assert bool((z.abs() < 8).all()), "a saturated sigmoid hides its pre-activation"
    if z.numel() > 1:
        assert float(z.std()) > 0.5


def test_nearest_index_table():
    """F.interpolate(mode="nearest") takes min(int(floorf(y * (float(h) / H))), h - 1); the integer formula (y * h) // H is another
    function unless H / h is an integer"""
    for n_in, n_out, differs in ((26, 88, [44]), (62, 112, [56]), (11, 88, []), (14, 112, []), (88, 88, []), (112, 112, []),
                                 (52, 88, [22, 44]), (104, 176, [22, 44, 88, 154])):
        scale = torch.tensor(n_in, dtype=torch.float32) / torch.tensor(n_out, dtype=torch.float32)
        want = torch.clamp(torch.floor(torch.arange(n_out, dtype=torch.float32) * scale).long(), max=n_in - 1)
        assert torch.equal(O.nearest_source_index(n_in, n_out), want)
        assert O.index_differences(n_in, n_out) == differs, (n_in, n_out, O.index_differences(n_in, n_out))

    def extra_channel(h, H, w, W):
        cells = torch.arange(h * w, dtype=torch.float64).view(1, h, w)  # every source cell its own value
        got = O.prep(torch.zeros((1, 1, H, W)), cells, torch.zeros_like(cells), True, 2)[0, :, :, 1]
        ys, xs = O.integer_source_index(h, H), O.integer_source_index(w, W)
        return got, cells[0][ys][:, xs]

    got, by_integers = extra_channel(26, 88, 62, 112)
    assert not torch.equal(got, by_integers)
    rows = (got != by_integers).all(dim=1).nonzero().flatten().tolist()  # a whole row moved, a whole column moved, nothing else
    cols = (got != by_integers).all(dim=0).nonzero().flatten().tolist()
    assert int((got != by_integers).sum()) == 88 + 112 - 1
    assert rows == O.index_differences(26, 88) and cols == O.index_differences(62, 112)
    for h, H, w, W in ((11, 88, 14, 112), (88, 88, 112, 112)):
        got, by_integers = extra_channel(h, H, w, W)
        assert torch.equal(got, by_integers)
    # the GPU file's maps at this ratio show the difference
    H, W, h, w = O.NONINTEGER_RATIO
    for pattern in O.NONINTEGER_PATTERNS:
        ops = O.noninteger_operands(pattern)
        sg = (ops["start"] + ops["goal"])[0]
        got = O.prep(ops["image"], ops["start"], ops["goal"], True, 2)[0, :, :, 1]
        assert torch.equal(got.float(), F.interpolate(sg.float()[None, None], size=(H, W), mode="nearest")[0, 0])
        assert not torch.equal(got, sg[O.integer_source_index(h, H)][:, O.integer_source_index(w, W)])
