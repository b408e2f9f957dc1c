"""The fp16 MFMA convolution (csrc/nastar_conv_flat.hip.h, nastar_conv3x3_f16), its 32x32 sibling (nastar_conv3x3_img32_f16) and the weight
gradient (csrc/nastar_conv_wgrad.hip.h, nastar_conv3x3_wgrad_f16) through the C ABI at their tile, chunk and segment edges, held to the BITS
of tests/mfma_conv_oracle.py: the operands are small integers for which fp32 accumulation is exact in any order (the oracle's precondition,
asserted again before every launch), so the only comparison is equality of the raw fp16 / fp32 bits.  The one inexact output, the sigmoid of
the FINAL epilogue, has an exact pre-activation: what is measured there is __expf alone.

Every call: outputs (out, out_f32, dw, the weight gradient's workspace) start as NaN with a sentinel run behind them in the same allocation
-- the run must survive, no NaN may remain (for the workspace: every partial tile of every split was written); every input (in, in2, dz, a)
is a 16-byte-aligned view into a larger allocation whose other elements, at least (W + 2) pixels each side, are NaN -- the kernels zero-fill
outside the tensor and never read there, a use of such an element would turn an output into NaN.

The shapes and what each reaches are listed in the oracle (CONV_CASES, IMG32_CASES, WGRAD_CASES).  With NASTAR_MFMA_EDGES_OUT=<file> one
record per case (route, precondition, differing elements, sigmoid errors) is written there as JSON (profiles/mfma_conv_edges.json is such a
run); nothing here reads it."""
import json
import os

import pytest
import torch

import mfma_conv_oracle as O

pytestmark = pytest.mark.gpu

NAN = float("nan")
TAIL, SENTINEL = 64, -7.0
# max |final_mul * sigmoid - float64| allowed at final_mul = 1 and 10: twice the largest error measured on an MI355X over the FINAL cases
# (7.02e-8 / 7.33e-7, profiles/mfma_conv_edges.json); the factor covers __expf at other arguments.  Far below the 1e-5 that
# test_flat_conv_final_layer_sigmoid demands of the same epilogue.
SIGMOID_BOUND = {1.0: 2 * 7.02e-8, 10.0: 2 * 7.33e-7}
FORM = "bit equality at every case with operands in {-2..2} x {-1,0,1}: the fp16 MFMA accumulates them exactly, no fallback was needed"
RECORDS = {}
_prepared = {}
_device_error = []  # a HIP error ends the GPU work of this file: later launches would run on a context that has faulted


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


def _lib():
    from neural_astar import _native
    return _native.load(), _native


def _stream():
    return torch.cuda.current_stream(_dev()).cuda_stream


@pytest.fixture(scope="module", autouse=True)
def _record():
    yield
    path = os.environ.get("NASTAR_MFMA_EDGES_OUT")
    if path and RECORDS:
        with open(path, "w") as f:
            json.dump(dict(form=FORM, sigmoid_bound={"final_mul=%g" % m: b for m, b in SIGMOID_BOUND.items()}, cases=RECORDS), f, indent=1,
                      sort_keys=True)


class Guarded:
    """an fp16 tensor as a 16-byte-aligned view inside a larger device allocation of NaNs"""

    def __init__(self, t16, margin):
        n, self.pre = t16.numel(), (margin + 7) // 8 * 8
        assert t16.dtype == torch.float16 and margin > 0
        self.buf = torch.full((self.pre + n + margin,), NAN, dtype=torch.float16, device=_dev())
        self.view = self.buf[self.pre:self.pre + n]
        self.view.copy_(t16.reshape(-1))
        self.ptr = self.view.data_ptr()
        assert self.ptr % 16 == 0 and not bool(torch.isnan(self.view).any())

    def check(self, what):
        n = self.view.numel()
        assert bool(torch.isnan(self.buf[:self.pre]).all()) and bool(torch.isnan(self.buf[self.pre + n:]).all()), what + ": a guard was written"


class Poisoned:
    """an output of n elements, NaN, with a sentinel run behind it in the same allocation"""

    def __init__(self, n, dtype):
        self.n = n
        self.buf = torch.empty((n + TAIL,), dtype=dtype, device=_dev())
        self.ptr = self.buf.data_ptr()
        self.poison()

    def poison(self):
        self.buf[:self.n] = NAN
        self.buf[self.n:] = SENTINEL

    def take(self, what):
        assert bool((self.buf[self.n:] == SENTINEL).all()), what + ": written past its end"
        body = self.buf[:self.n].clone()
        left = int(torch.isnan(body).sum())
        assert left == 0, "%s: %d of %d elements are NaN -- never written, or made from a guard element" % (what, left, self.n)
        return body


def _synchronize(native, rc, what):
    try:
        native.check(rc, what)
        torch.cuda.synchronize()
    except Exception as e:
        _device_error.append("%s: %s" % (what, e))
        raise


def _ready():
    assert not _device_error, "not launched: an earlier call ended in a device error (%s)" % _device_error[0]


def _f32(t):
    f = t.float()
    assert torch.equal(f.double(), t)
    return f.to(_dev()).contiguous()


def _same_bits(got, want, what):
    """bit equality of a device tensor and the oracle's: (number of differing elements, a message naming the first one)"""
    assert got.shape == want.shape and got.dtype == want.dtype, what
    ints = {torch.float16: torch.int16, torch.float32: torch.int32}[got.dtype]
    g, w = got.cpu().contiguous().view(ints), want.contiguous().view(ints)
    bad = g != w
    n = int(bad.sum())
    if n:
        first = bad.nonzero()[0].tolist()
        return n, "%s: %d of %d elements differ, first at %s: got %r, want %r" % (what, n, bad.numel(), first, float(got.cpu()[tuple(first)]),
                                                                                 float(want[tuple(first)]))
    return 0, ""


# ---- the convolution ------------------------------------------------------------------------------------------------------------------------
def _conv_case(case):
    """operands, oracle output and precondition of a case: computed once"""
    if case not in _prepared:
        ops = O.conv_operands(case)
        _prepared[case] = (ops, O.conv_forward(ops), O.conv_precondition(ops))
    return _prepared[case]


def _launch_conv(case, ops, pre, final_mul=1.0, img32=False):
    """one call of nastar_conv3x3_f16 (or nastar_conv3x3_img32_f16): fp16 [B,H,W,cout (x2)] or fp32 [B,H,W], after every buffer check"""
    _ready()
    lib, native = _lib()
    c, M = case, 2 if case.split else 1
    assert max(pre) < O.EXACT_LIMIT, "operands that can round in fp32 prove nothing here"
    what = O.conv_id(c)
    a = Guarded(O.planes(ops["in_hi"], ops["in_lo"], c.split), (c.W + 2) * c.c1 * M)
    b = Guarded(O.planes(ops["in2_hi"], ops["in2_lo"], c.split), (c.W + 2) * c.c2 * M) if c.c2 else None
    wpack = O.pack_weights(ops["wseg"], c.split).to(_dev()).contiguous()
    assert wpack.numel() == 9 * (3 if c.split else 1) * (c.c1 + c.c2) * c.cout  # the buffers the kernel indexes without a bound of their own
    scale, shift = _f32(ops["scale"]), _f32(ops["shift"])
    assert scale.numel() == shift.numel() == c.cout
    npix = c.B * c.H * c.W
    out = Poisoned(npix if c.final else npix * c.cout * M, torch.float32 if c.final else torch.float16)
    if img32:
        assert (c.H, c.W, c.c2, c.ups, c.final) == (32, 32, 0, False, "")
        rc = lib.nastar_conv3x3_img32_f16(a.ptr, wpack.data_ptr(), scale.data_ptr(), shift.data_ptr(), out.ptr, c.B, c.c1, c.cout,
                                          O.conv_flags(c), _stream())
    else:
        rc = lib.nastar_conv3x3_f16(a.ptr, b.ptr if b else None, wpack.data_ptr(), scale.data_ptr(), shift.data_ptr(),
                                    None if c.final else out.ptr, out.ptr if c.final else None, c.B, c.H, c.W, c.c1, c.c2, c.cout,
                                    O.conv_flags(c), float(final_mul), _stream())
    _synchronize(native, rc, "nastar_conv3x3_f16 " + what)
    body = out.take(what)
    for t in (a, b):
        if t is not None:
            t.check(what)
    return body.view(c.B, c.H, c.W) if c.final else body.view(c.B, c.H, c.W, c.cout * M)


def _check_conv(case, img32=False):
    ops, want, pre = _conv_case(case)
    got = _launch_conv(case, ops, pre, img32=img32)
    what = O.conv_id(case) + (" img32" if img32 else "")
    if case.final:
        pairs = [("out_f32", got, want["f32"].float())]
        assert torch.equal(pairs[0][2].double(), want["f32"])
    else:
        pairs = [("hi", got[..., :case.cout], want["hi"])] + ([("lo", got[..., case.cout:], want["lo"])] if case.split else [])
    differing, messages = 0, []
    for name, g, w in pairs:
        n, msg = _same_bits(g.contiguous(), w, what + " " + name)
        differing += n
        messages.append(msg)
    route = dict(O.conv_geometry(case), kernel="img32") if img32 else O.conv_geometry(case)
    RECORDS[("img32 " if img32 else "conv ") + O.conv_id(case)] = dict(route=route, precondition=max(pre), differing=differing)
    assert differing == 0, "; ".join(m for m in messages if m)
    if not case.final:
        assert not bool(got[..., case.cout - 3:case.cout].any()), "padded output channels (scale = shift = 0) are not zero"
    return got


@pytest.mark.parametrize("case", [c for c in O.CONV_CASES if c.final != "sig"], ids=O.conv_id)
def test_convolution_has_the_oracles_bits(case):
    _check_conv(case)


@pytest.mark.parametrize("case", O.IMG32_CASES, ids=O.conv_id)
def test_img32_layer_has_the_oracles_bits(case):
    _check_conv(case, img32=True)


@pytest.mark.parametrize("mul", O.FINAL_MULS)
@pytest.mark.parametrize("case", [c for c in O.CONV_CASES if c.final == "sig"], ids=O.conv_id)
def test_final_sigmoid_is_expf_away_from_float64(case, mul):
    ops, _, pre = _conv_case(case)
    want = O.conv_forward(ops, final_mul=mul)
    got = _launch_conv(case, ops, pre, final_mul=mul)
    err = float((got.cpu().double() - want["f32"]).abs().max())
    z = want["z"]
    print(f"SIGMOID {O.conv_id(case)} final_mul={mul}: max |out_f32 - float64| = {err:.3e} (pre-activation in [{float(z.min()):.2f}, {float(z.max()):.2f}])")
    rec = RECORDS.setdefault("conv " + O.conv_id(case), dict(route=O.conv_geometry(case), precondition=max(pre), differing=0, sigmoid_error={}))
    rec["sigmoid_error"]["final_mul=%g" % mul] = err
    assert SIGMOID_BOUND[mul] <= 1e-5
    assert err <= SIGMOID_BOUND[mul], err


# ---- the weight gradient --------------------------------------------------------------------------------------------------------------------
def _wgrad_case(case):
    if case not in _prepared:
        ops = O.wgrad_operands(case)
        _prepared[case] = (ops, O.conv_wgrad(ops), O.wgrad_precondition(ops))
    return _prepared[case]


@pytest.mark.parametrize("case", O.WGRAD_CASES, ids=O.wgrad_id)
def test_weight_gradient_has_the_oracles_bits(case):
    _ready()
    lib, native = _lib()
    c, M = case, 2 if case.split else 1
    ops, want, pre = _wgrad_case(c)
    what = O.wgrad_id(c)
    geo = O.wgrad_geometry(c.B, c.H, c.W, c.co, c.ci)
    nbytes = int(lib.nastar_conv3x3_wgrad_workspace_bytes(c.B, c.H, c.W, c.co, c.ci))
    tile_bytes = 9 * c.co * c.ci * 4
    assert nbytes % tile_bytes == 0
    nsplit = nbytes // tile_bytes
    assert nsplit == geo["nsplit"], "the oracle's mirror of the split count is stale"
    assert pre < O.EXACT_LIMIT, "operands that can round in fp32 prove nothing here"
    dz = Guarded(O.planes(ops["dz_hi"], ops["dz_lo"], c.split), (c.W + 2) * c.co * M)
    a = Guarded(O.planes(ops["a_hi"], ops["a_lo"], c.split), (c.W + 2) * c.ci * M)
    dw = Poisoned(c.co_real * c.ci_real * 9, torch.float32)
    ws = Poisoned(nbytes // 4, torch.float32)
    gscale = None if c.gscale is None else torch.full((1,), c.gscale, dtype=torch.float32, device=_dev())
    runs = []
    for _ in range(2):  # twice: fixed-order partial sums, bitwise equal
        dw.poison()
        ws.poison()
        rc = lib.nastar_conv3x3_wgrad_f16(dz.ptr, a.ptr, dw.ptr, c.B, c.H, c.W, c.co, c.ci, c.co_real, c.ci_real, int(c.split),
                                          float(c.out_scale), None if gscale is None else gscale.data_ptr(), ws.ptr, nbytes, _stream())
        _synchronize(native, rc, "nastar_conv3x3_wgrad_f16 " + what)
        ws.take(what + " workspace")  # no NaN left: every partial tile of every split was written
        runs.append(dw.take(what + " dw").view(c.co_real, c.ci_real, 3, 3))
        dz.check(what)
        a.check(what)
    want32 = want.float()
    assert torch.equal(want32.double(), want)
    differing, msg = _same_bits(runs[0], want32, what)
    route = {k: geo[k] for k in ("seg", "nseg", "ragged", "R", "G", "NP", "KS", "nchunk", "COB", "CIB", "staging")}
    RECORDS["wgrad " + what] = dict(route=dict(route, nsplit=nsplit), precondition=pre, differing=differing)
    assert differing == 0, msg
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32)), "two calls differ"


def test_weight_gradient_support_sweep():
    """host calls only: workspace_bytes == 0 exactly where the oracle's chunk_rows says unsupported; W = 1 is refused by the entry point"""
    _ready()
    lib, _ = _lib()
    for H in range(1, 41):
        for W in range(1, 301):
            nbytes = int(lib.nastar_conv3x3_wgrad_workspace_bytes(1, H, W, 32, 32))
            assert (nbytes == 0) == (O.chunk_rows(H, W) == 0), (H, W, nbytes)
    t = torch.zeros((4096,), dtype=torch.float32, device=_dev())
    rc = lib.nastar_conv3x3_wgrad_f16(t.data_ptr(), t.data_ptr(), t.data_ptr(), 2, 5, 1, 32, 32, 32, 32, 0, 1.0, None, t.data_ptr(), 4096 * 4,
                                      _stream())
    assert rc == 2, rc  # NASTAR_ERR_UNSUPPORTED
