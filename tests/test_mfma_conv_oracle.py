"""tests/mfma_conv_oracle.py checked on the CPU: the restated convolution and weight gradient against torch in float64, the weight pack
against the package's own packer, the geometry mirrors against neural_astar.encoder_train, the exactness precondition at every case of
tests/test_mfma_conv_edges_gpu.py (the lists are the oracle's: one place), and the defects (a)-(p): each must change the oracle's own
output at EVERY listed case it applies to, and each must have such a case -- otherwise the integer operands would not excite that fault
and the GPU test's bit comparison would not see it."""
import functools

import pytest
import torch
import torch.nn.functional as F

import mfma_conv_oracle as O

ALL_CONV = O.CONV_CASES + O.IMG32_CASES


@functools.lru_cache(maxsize=None)
def _conv(case):
    ops = O.conv_operands(case)
    return ops, O.conv_forward(ops)


@functools.lru_cache(maxsize=None)
def _wgrad(case):
    ops = O.wgrad_operands(case)
    return ops, O.conv_wgrad(ops)


# ---- the oracle against torch -------------------------------------------------------------------------------------------------------------
def _float_ops(case, seed):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(s, generator=g, dtype=torch.float64)
    hw1 = (case.H // 2, case.W // 2) if case.ups else (case.H, case.W)
    cin = case.c1 + case.c2
    return dict(case=case, in_hi=rnd(case.B, *hw1, case.c1), in_lo=rnd(case.B, *hw1, case.c1) * 1e-3,
                in2_hi=rnd(case.B, case.H, case.W, case.c2) if case.c2 else None,
                in2_lo=rnd(case.B, case.H, case.W, case.c2) * 1e-3 if case.c2 else None,
                wseg=[rnd(case.cout, cin, 3, 3) for _ in range(3)], scale=rnd(case.cout), shift=rnd(case.cout))


def _torch_input(ops, plane):
    case = ops["case"]
    nchw = lambda t: t.permute(0, 3, 1, 2)
    x = nchw(ops["in_" + plane])
    if case.ups:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    if case.c2:
        x = torch.cat((x, nchw(ops["in2_" + plane])), dim=1)
    return x


FLOAT_CASES = [O.ConvCase(2, 5, 7, 32, 0, 32, False, False, True, "", False), O.ConvCase(3, 4, 6, 32, 64, 64, True, False, False, "", False),
               O.ConvCase(2, 6, 4, 64, 32, 32, True, True, True, "", False), O.ConvCase(2, 1, 5, 32, 0, 32, False, True, False, "raw", False),
               O.ConvCase(1, 3, 1, 32, 0, 32, False, False, False, "sig", False)]


@pytest.mark.parametrize("case", FLOAT_CASES, ids=O.conv_id)
def test_conv_forward_is_conv2d_of_the_concatenated_upsampled_input(case):
    ops = _float_ops(case, 3)
    xh = _torch_input(ops, "hi")
    ref = F.conv2d(xh, ops["wseg"][0], None, padding=1)
    if case.split:
        ref = ref + F.conv2d(_torch_input(ops, "lo"), ops["wseg"][1], None, padding=1) + F.conv2d(xh, ops["wseg"][2], None, padding=1)
    ref = ref * ops["scale"].view(1, -1, 1, 1) + ops["shift"].view(1, -1, 1, 1)
    got = O.conv_value(ops)
    if case.final:
        ref = ref[:, 0]
        if case.final == "sig":
            ref, got = 7.0 * torch.sigmoid(ref), O.conv_forward(ops, final_mul=7.0)["f32"]
    else:
        ref = (ref.clamp_min(0) if case.relu else ref).permute(0, 2, 3, 1)
    assert got.shape == ref.shape
    assert float((got - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))


def test_split_forward_is_the_full_product_minus_the_lo_lo_term():
    case = O.ConvCase(2, 4, 5, 32, 0, 32, False, True, False, "", False)
    ops = _float_ops(case, 5)
    w = ops["wseg"][0]
    w_hi = w.half().double()
    ops["wseg"] = [w_hi, w_hi, w - w_hi]
    ops["scale"], ops["shift"] = torch.ones(32, dtype=torch.float64), torch.zeros(32, dtype=torch.float64)
    conv = lambda x, k: F.conv2d(x.permute(0, 3, 1, 2), k, None, padding=1).permute(0, 2, 3, 1)
    full, lolo = conv(ops["in_hi"] + ops["in_lo"], w), conv(ops["in_lo"], w - w_hi)
    assert float(lolo.abs().max()) > 0
    assert float((O.conv_value(ops) - (full - lolo)).abs().max()) <= 1e-12 * float(full.abs().max())


def test_clamp_and_rounding_of_the_epilogue():
    case = O.ConvCase(1, 1, 1, 32, 0, 32, False, True, False, "", False)
    ops = O.conv_operands(case)
    ops["scale"] = torch.zeros(32, dtype=torch.float64)
    ops["shift"] = torch.tensor([70000.0, -70000.0, 2049.0, 2051.0, -4099.0, 0.5] + [0.0] * 26, dtype=torch.float64)
    out = O.conv_forward(ops)
    assert out["hi"][0, 0, 0, :6].tolist() == [65504.0, -65504.0, 2048.0, 2052.0, -4100.0, 0.5]   # ties to even; 4099 is nearer 4100
    assert out["lo"][0, 0, 0, :6].tolist() == [0.0, 0.0, 1.0, -1.0, 1.0, 0.0]


@pytest.mark.parametrize("split", [False, True])
def test_conv_wgrad_is_autograd_of_conv2d(split):
    case = O.WgradCase(3, 5, 7, 64, 32, 61, 27, split, 0.5, 8.0)
    g = torch.Generator().manual_seed(11)
    rnd = lambda ch, s=1.0: torch.randn((3, 5, 7, ch), generator=g, dtype=torch.float64) * s
    ops = dict(case=case, dz_hi=rnd(64), dz_lo=rnd(64, 1e-3), a_hi=rnd(32), a_lo=rnd(32, 1e-3))
    nchw = lambda t: t.permute(0, 3, 1, 2)

    def grad(a, dz):
        w = torch.zeros((64, 32, 3, 3), dtype=torch.float64, requires_grad=True)
        F.conv2d(nchw(a), w, None, padding=1).backward(nchw(dz))
        return w.grad

    ref = grad(ops["a_hi"], ops["dz_hi"])
    if split:
        ref = ref + grad(ops["a_hi"], ops["dz_lo"]) + grad(ops["a_lo"], ops["dz_hi"])
    ref = ref[:61, :27] * (0.5 / 8.0)
    got = O.conv_wgrad(ops)
    assert got.shape == ref.shape
    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


@pytest.mark.parametrize("split", [False, True])
def test_weight_pack_agrees_with_the_packages_packer(split):
    """written from include/nastar.h's wpack[tap][v/8][n][v%8]; compared once with encoder_hip.pack_conv_weight"""
    from neural_astar import encoder_hip as E
    g = torch.Generator().manual_seed(2)
    wseg = [torch.randint(-1, 2, (64, 96, 3, 3), generator=g).double() for _ in range(3)]
    mine = O.pack_weights(wseg, split)
    V = 96 * (3 if split else 1)
    assert mine.shape == (9, V // 8, 64, 8) and mine.dtype == torch.float16
    theirs = E.pack_conv_weight(torch.cat(wseg[:3 if split else 1], dim=1).float(), V, 64, torch.float16)
    assert torch.equal(mine.view(torch.int16), theirs)
    # element by element, as the header words it
    for tap, v, n in ((0, 0, 0), (4, 95, 63), (8, V - 1, 17), (5, V // 2, 40)):
        seg, c = divmod(v, 96)
        assert float(mine[tap, v // 8, n, v % 8]) == float(wseg[seg][n, c, tap // 3, tap % 3])


# ---- geometry mirrors ---------------------------------------------------------------------------------------------------------------------
def test_weight_gradient_geometry_mirrors_agree_with_the_package():
    from neural_astar import encoder_train as T
    for W in range(1, 401):
        assert O.wgrad_segment(W) == T.wgrad_segment(W), W
        for H in range(1, 65):
            assert O.chunk_rows(H, W) == T.chunk_rows(H, W), (H, W)


def test_the_listed_shapes_take_the_routes_their_comments_name():
    geo = lambda *s: O.wgrad_geometry(*s)
    assert geo(1, 1, 2, 32, 32)["G"] == 16 and geo(17, 1, 2, 32, 32)["nchunk"] == 2
    g = geo(11, 3, 3, 64, 32)
    assert g["G"] == 8 and O.WG_MAX_PIX // 9 == 10 and g["COB"] == 2 and g["nchunk"] == 2
    g = geo(3, 2, 24, 32, 64)
    assert g["G"] == 1 and g["R"] == 2 and g["CIB"] == 2
    g = geo(2, 53, 2, 32, 32)
    assert (g["R"], g["NP"], g["KS"], g["nchunk"]) == (1, 2, 1, 106)
    g = geo(1, 7, 13, 32, 32)
    assert (g["R"], g["NP"], g["KS"]) == (7, 91, 6)
    for shape, n in O.WGRAD_NSPLIT.items():
        assert geo(*shape)["nsplit"] == n
    assert [geo(1, 2, W, 32, 32)["staging"] for W in (64, 65, 96)] == ["narrow", "wide", "wide"]
    g = geo(2, 2, 97, 32, 32)
    assert (g["seg"], g["nseg"], g["ragged"]) == (49, 2, True)
    g = geo(1, 2, 194, 32, 64)
    assert (g["seg"], g["nseg"], g["ragged"]) == (65, 3, True)
    assert geo(1, 2, 192, 64, 32)["seg"] == 96 and geo(2, 3, 128, 32, 32)["seg"] == 64
    g = geo(2, 4, 4, 96, 160)
    assert (g["COB"], g["CIB"], g["tiles"]) == (1, 1, 15)
    cg = {(c.B, c.H, c.W, c.split): O.conv_geometry(c) for c in O.CONV_CASES}
    assert cg[65, 2, 2, False] == dict(mode="flat", NT=32, ntiles=2, slices=2)
    assert cg[3, 28, 28, True] == dict(mode="flat", NT=64, ntiles=10, slices=3)
    assert cg[2, 3, 126, False]["mode"] == "flat" and cg[2, 1, 127, False]["mode"] == "wide"
    assert cg[2, 5, 129, True]["ntiles"] == 2 * 2 * 3
    assert cg[3, 2, 2, False]["slices"] == 32 and cg[2, 4, 6, True]["slices"] == 9


# ---- the precondition at every case the GPU test runs ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL_CONV, ids=O.conv_id)
def test_conv_precondition_holds(case):
    ops, out = _conv(case)
    acc, v = O.conv_precondition(ops)
    assert 0 < acc < O.EXACT_LIMIT and v < O.EXACT_LIMIT, (acc, v)
    if case.clamp:  # the clamp is on the path, on both sides, and some residual below it is negative
        assert float(out["v"].max()) == O.F16_MAX and float(out["v"].min()) == (0.0 if case.relu else -O.F16_MAX)
        raw = O.conv_acc(ops) * ops["scale"] + ops["shift"]
        assert float(raw.abs().max()) > O.F16_MAX
        if case.split:
            assert float(out["lo"].min()) < 0 < float(out["lo"].max())
    elif case.final:
        assert float(out["z"].min()) < -4 and float(out["z"].max()) > 4  # the sigmoid is exercised over its range ...
        assert float(out["z"].abs().min()) < 1                            # ... and around zero
    else:
        assert float(out["hi"][..., -3:].abs().max()) == 0, "padded output channels (scale = shift = 0)"
        assert bool(ops["wseg"][0][-3:].any())


@pytest.mark.parametrize("case", O.WGRAD_CASES, ids=O.wgrad_id)
def test_wgrad_precondition_holds(case):
    ops, dw = _wgrad(case)
    assert 0 < O.wgrad_precondition(ops) < O.EXACT_LIMIT
    assert torch.equal(dw.float().double(), dw) and dw.shape == (case.co_real, case.ci_real, 3, 3)


# ---- the defects -----------------------------------------------------------------------------------------------------------------------------
def _applicable(defects, cases, letter):
    return [c for c in cases if defects[letter][1](c)]


@pytest.mark.parametrize("letter", sorted(O.CONV_DEFECTS))
def test_every_convolution_defect_changes_the_bits_wherever_it_applies(letter):
    cases = _applicable(O.CONV_DEFECTS, ALL_CONV, letter)
    assert cases, "defect (%s) %s: no case applies" % (letter, O.CONV_DEFECTS[letter][0])
    for case in cases:
        ops, clean = _conv(case)
        assert O.conv_differs(clean, O.conv_forward(ops, defect=letter)), "(%s) is invisible at %s" % (letter, O.conv_id(case))


@pytest.mark.parametrize("letter", sorted(O.WGRAD_DEFECTS))
def test_every_weight_gradient_defect_changes_the_bits_wherever_it_applies(letter):
    cases = _applicable(O.WGRAD_DEFECTS, O.WGRAD_CASES, letter)
    assert cases, "defect (%s) %s: no case applies" % (letter, O.WGRAD_DEFECTS[letter][0])
    for case in cases:
        ops, clean = _wgrad(case)
        bad = O.conv_wgrad(ops, defect=letter)
        if letter == "p":  # the padded tensor holds non-zeros beyond the crop: written, they would land outside dw
            beyond = bad.clone()
            beyond[:case.co_real, :case.ci_real] = 0
            assert bool(beyond.any()), O.wgrad_id(case)
            assert torch.equal(bad[:case.co_real, :case.ci_real], clean)
        else:
            assert O.wgrad_differs(clean, bad), "(%s) is invisible at %s" % (letter, O.wgrad_id(case))


def test_the_defect_lists_are_the_issues():
    assert sorted(O.CONV_DEFECTS) == list("abcdefghi") and sorted(O.WGRAD_DEFECTS) == list("jklmnop")
