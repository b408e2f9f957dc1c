"""CPU, no device: the layout helpers of tests/field_layouts.py, which tests/test_field_layouts_gpu.py hands to every entry point of the field
family.  On CPU tensors every layout shows exactly the given values, has the pointer / stride property it is named for, and has its
poison where it is said to be; and the combinations the GPU test runs are the ones listed here.
"""
import numpy as np
import pytest
import torch

import field_layouts as FL

f32 = np.float32
SHAPES = sorted(set(FL.EXACT_SHAPES + FL.TILED_SHAPES + FL.SOFT_SHAPES + FL.SOFT_TILED_SHAPES))


def _vals(*shape):
    return (1 + np.arange(int(np.prod(shape)), dtype=f32)).reshape(shape)  # every cell its own finite value


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("layout", FL.MAP_LAYOUTS)
@pytest.mark.parametrize("H,W", SHAPES)
def test_every_map_layout_shows_the_values_and_poison_beside_them(H, W, layout):
    v = _vals(FL.B, H, W)
    t, base = FL.laid_out(v, layout)
    see = FL.shown(t)
    assert tuple(see.shape) == (FL.B, H, W) and see.dtype == torch.float32 and _bits(see, torch.from_numpy(v))
    rest = FL.beside(see, base)
    assert bool(torch.isnan(rest).all())
    assert (rest.numel() == 0) == (layout == "fresh"), "every layout but the control has poison beside its view"
    if layout == "fresh":
        assert t.is_contiguous() and t.data_ptr() % 16 == 0
    elif layout in FL.MISALIGNED:
        k = int(layout[-1])
        assert t.is_contiguous() and t.data_ptr() % 16 == 4 * k
        assert bool(torch.isnan(base[:k]).all()) and bool(torch.isnan(base[k + v.size:]).all()) and base.numel() - k - v.size >= 3
    elif layout == "tail":
        assert t.is_contiguous() and (H * W) % 2 == 1 and t.data_ptr() % 16 == (4 * H * W) % 16 != 0     # the natural misaligned case
        assert bool(torch.isnan(base[0]).all()) and t.data_ptr() == base[1].data_ptr()
    elif layout == "channel0":
        assert tuple(t.shape) == (FL.B, 2, H, W) and t.is_contiguous() and bool(torch.isnan(t[:, 1]).all())
    elif layout == "transposed":
        assert t.stride() == ((W + 1) * H, 1, H) and not t.is_contiguous() and bool(torch.isnan(base[:, W]).all())
    elif layout == "rowpad":
        assert t.stride() == (H * (W + 3), W + 3, 1) and not t.is_contiguous() and bool(torch.isnan(base[..., W:]).all())


@pytest.mark.parametrize("H,W", SHAPES)
def test_broadcast_stride0_and_the_gradient_layouts(H, W):
    one = np.repeat(_vals(1, H, W), FL.B, axis=0)
    t, base = FL.laid_out(one, "broadcast")
    assert t.stride() == (0, W, 1) and not t.is_contiguous() and _bits(t, torch.from_numpy(one))
    assert bool(torch.isnan(FL.beside(t, base)).all()) and FL.beside(t, base).numel() == FL.B * H * W
    with pytest.raises(AssertionError, match="all the same"):
        FL.laid_out(_vals(FL.B, H, W), "broadcast")
    g = FL.stride0(0.75, FL.B, H, W)
    assert tuple(g.shape) == (FL.B, 1, H, W) and g.stride(0) == g.stride(3) == 0 and not g.is_contiguous() and bool((g == 0.75).all())
    v = _vals(FL.B, H, W)
    for layout in FL.GRAD_LAYOUTS:
        u = FL.lay(v, layout)
        assert u.numel() == v.size and tuple(u.shape[-2:]) == (H, W) and _bits(u.reshape(FL.B, H, W), torch.from_numpy(v)), layout
    assert tuple(FL.lay(v, "unsqueezed").shape) == (FL.B, 1, H, W)
    p = _vals(FL.B, 8, H, W)
    for layout in FL.POLICY_GRAD_LAYOUTS:
        u, base = FL.laid_out(p, layout)
        assert tuple(u.shape) == (FL.B, 8, H, W) and _bits(u, torch.from_numpy(p)), layout
        assert u.is_contiguous() == (layout == "fresh") and bool(torch.isnan(FL.beside(u, base)).all())
    assert FL.lay(p, "permuted").stride() == (8 * H * W, 1, 8 * W, 8)
    assert FL.lay(p, "rowpad").stride() == (8 * H * (W + 3), H * (W + 3), W + 3, 1)


def test_the_values_are_copied_so_a_shared_case_is_never_written():
    v = _vals(FL.B, 5, 7)
    v.setflags(write=False)
    for layout in FL.MAP_LAYOUTS:
        FL.shown(FL.lay(v, layout)).mul_(2)
    assert np.array_equal(v, _vals(FL.B, 5, 7))


def test_the_combinations_the_gpu_test_runs():
    """shape x layout; one input in a layout and the other two fresh, each of the three in that position in turn; all three together"""
    combos = FL.input_combinations()
    others = [name for name in FL.MAP_LAYOUTS if name != "fresh"]
    assert len(combos) == len(set(combos)) == 4 * len(others) and ("fresh",) * 3 not in combos
    for name in others:
        assert (name,) * 3 in combos
        for slot in range(3):
            assert tuple(name if k == slot else "fresh" for k in range(3)) in combos
    # the conjunction behind the ``vec`` flag of the two kernels with vector loads: cost aligned and goal shift1, and its two siblings
    for case in (("fresh", "shift1", "fresh"), ("shift1", "fresh", "fresh"), ("fresh", "fresh", "shift1")):
        assert case in combos
    more = FL.input_combinations(broadcast=True)
    assert more[:len(combos)] == combos and set(more[len(combos):]) == {("fresh", "broadcast", "fresh"), ("fresh", "fresh", "broadcast"),
                                                                           ("fresh", "broadcast", "broadcast")}
    assert all(c[0] != "broadcast" for c in more), "only goal and obstacle maps are broadcast"
    assert FL.B == 3 and all((H * W) % 2 == 1 for H, W in SHAPES), "an odd H*W: tail and the per-map bases misalign"
    assert FL.EXACT_SHAPES == ((5, 7), (33, 33), (65, 65)) and FL.TILED_SHAPES == ((65, 65), (1, 197))
    assert FL.SOFT_SHAPES == ((5, 7), (31, 33)) and FL.SOFT_TILED_SHAPES == ((65, 65),) and FL.MASKS == (0x1EF, 0x0EB)
