"""The tensors a caller may hand the field ops (``ops.cost_to_go`` ... ``ops.soft_policy_nll``) instead of a fresh contiguous one: from ONE numpy
array of values, torch tensors in named layouts.  Every layout shows the same values; the bytes beside the view hold NaN, which is loud
in all three roles -- as a cost on a passable cell it is BAD_COST, as a goal a non-zero extra goal, as a passable value an open obstacle.

Shared by tests/test_field_layouts.py (CPU: the helpers themselves) and tests/test_field_layouts_gpu.py; no device is needed to import it.
"""
import numpy as np
import torch

f32 = np.float32
POISON = float("nan")

# the layouts of a map-shaped input ([B,H,W] values); ``broadcast`` beside them, for batches whose maps are all the same map
MAP_LAYOUTS = ("fresh", "shift1", "shift2", "shift3", "tail", "channel0", "transposed", "rowpad")
MISALIGNED = ("shift1", "shift2", "shift3")  # 4, 8 and 12 bytes past a 16-byte boundary at every shape (``tail`` too when H*W is odd)
# the layouts of an upstream gradient of ``dists`` / ``paths`` ([B,H,W] values; ``stride0`` shows one constant)
GRAD_LAYOUTS = ("fresh", "unsqueezed", "transposed", "rowpad", "shift1")
# ... and of ``grad_log_policies`` ([B,8,H,W] values)
POLICY_GRAD_LAYOUTS = ("fresh", "permuted", "rowpad")


def _values(values, device):
    a = np.ascontiguousarray(values, f32)
    return torch.from_numpy(a.copy()).to(device)


def _poisoned(shape, device):
    base = torch.full(tuple(shape), POISON, dtype=torch.float32, device=device)
    assert base.data_ptr() % 16 == 0, "a fresh allocation is 16-byte aligned"
    return base


def laid_out(values, layout: str, device="cpu"):
    """``values`` (numpy, any shape with a leading batch axis) -> ``(tensor, base)``: the tensor to hand to an op and the whole buffer it
    was carved from (poison wherever the tensor does not look).  ``shown(tensor)`` is what an op reads of it."""
    v = _values(values, device)
    shape, n = tuple(v.shape), v.numel()
    if layout == "fresh":
        assert v.is_contiguous() and v.data_ptr() % 16 == 0
        return v, v
    if layout in MISALIGNED:  # contiguous, carved out of a flat buffer at an element offset of 1, 2 or 3
        k = int(layout[-1])
        base = _poisoned((k + n + 4,), device)
        base[k:k + n] = v.reshape(-1)
        t = base[k:k + n].view(shape)
        assert t.is_contiguous() and t.data_ptr() % 16 == 4 * k, (layout, t.data_ptr() % 16)
        return t, base
    if layout == "tail":  # big[1:] of a batch whose map 0 is poison: misaligned whenever the cells of one map are no multiple of 4
        base = _poisoned((shape[0] + 1,) + shape[1:], device)
        base[1:] = v
        t = base[1:]
        assert t.is_contiguous() and t.data_ptr() % 16 == (4 * (n // shape[0])) % 16, (layout, t.data_ptr() % 16)
        return t, base
    if layout == "channel0":  # [B,2,H,W], passed as it is: the ops take channel 0
        assert v.ndim == 3, "channel0 is a layout of [B,H,W] values"
        base = _poisoned((shape[0], 2) + shape[1:], device)
        base[:, 0] = v
        assert base.ndim == 4 and base.shape[1] == 2 and base.is_contiguous() and bool(torch.isnan(base[:, 1]).all())
        return base, base
    if layout == "broadcast":  # one map .expand()ed over the batch
        assert (np.asarray(values) == np.asarray(values)[:1]).all(), "broadcast is a layout of batches whose maps are all the same"
        base = _poisoned((shape[0] + 1,) + shape[1:], device)  # (B poison-or-map planes from the map on: a flat read of B maps stays inside)
        base[1] = v[0]
        t = base[1:2].expand(shape)
        assert t.stride(0) == 0 and (shape[0] == 1 or not t.is_contiguous()), (layout, t.stride())
        return t, base
    if layout == "transposed":  # [..., W, H] viewed as [..., H, W]; one more (poison) row behind the W rows of every map
        H, W = shape[-2:]
        base = _poisoned(shape[:-2] + (W + 1, H), device)
        base[..., :W, :] = v.transpose(-1, -2)
        t = base[..., :W, :].transpose(-1, -2)
        assert tuple(t.shape) == shape and t.stride(-1) == H and t.stride(-2) == 1 and (n == shape[0] or not t.is_contiguous()), (layout, t.stride())
        return t, base
    if layout == "rowpad":  # three poison cells behind every row
        W = shape[-1]
        base = _poisoned(shape[:-1] + (W + 3,), device)
        base[..., :W] = v
        t = base[..., :W]
        assert t.stride(-2) == W + 3 and t.stride(-1) == 1 and not t.is_contiguous(), (layout, t.stride())
        return t, base
    if layout == "unsqueezed":  # [B,1,H,W], contiguous: the shape of ``dists`` and ``paths``
        assert v.ndim == 3
        t = v[:, None]
        assert tuple(t.shape) == (shape[0], 1) + shape[1:] and t.is_contiguous()
        return t, v
    if layout == "permuted":  # [B,8,H,W] permuted from [B,H,W,8]
        assert v.ndim == 4
        base = v.permute(0, 2, 3, 1).contiguous()
        t = base.permute(0, 3, 1, 2)
        assert tuple(t.shape) == shape and t.stride(1) == 1 and t.stride(-1) == shape[1] and (n == shape[0] or not t.is_contiguous()), (layout, t.stride())
        return t, base
    raise ValueError(f"unknown layout {layout!r}")


def lay(values, layout: str, device="cpu") -> torch.Tensor:
    return laid_out(values, layout, device)[0]


def stride0(value: float, B: int, H: int, W: int, device="cpu") -> torch.Tensor:
    """the upstream gradient autograd hands a sum's backward: one constant, stride 0 on every axis longer than 1, [B,1,H,W]"""
    t = torch.full((1, 1, 1, 1), float(value), dtype=torch.float32, device=device).expand(B, 1, H, W)
    assert all(s == 0 for s, n in zip(t.stride(), t.shape) if n > 1) and (B * H * W == 1 or not t.is_contiguous())
    return t


def shown(t: torch.Tensor) -> torch.Tensor:
    """what an op reads of a map-shaped argument: channel 0 of a [B,C,H,W] tensor, the tensor itself otherwise (``ops._maps3``)"""
    return t[:, 0] if t.ndim == 4 else t


def beside(t: torch.Tensor, base: torch.Tensor) -> torch.Tensor:
    """the elements of ``base`` that ``t`` (a view into it) does not look at, flat -- for a ``channel0`` tensor pass ``shown(t)``"""
    assert t.untyped_storage().data_ptr() == base.untyped_storage().data_ptr() and base.is_contiguous()
    cells = torch.arange(base.numel(), device=base.device)
    seen = torch.as_strided(cells, tuple(t.shape), t.stride(), t.storage_offset() - base.storage_offset())
    looked = torch.zeros(base.numel(), dtype=torch.bool, device=base.device)
    looked[seen.reshape(-1)] = True
    return base.reshape(-1)[~looked]


def input_combinations(layouts=MAP_LAYOUTS, broadcast: bool = False):
    """the (cost, goal, passable) layout triples a GPU test runs beside ("fresh", "fresh", "fresh"): every other layout on one input at a
    time -- each of the three in the non-fresh position in turn, so the conjunction behind a kernel's ``vec`` flag is broken by each of
    its pointers alone -- and on all three together.  ``broadcast``: the goal and the obstacle map broadcast too, alone and together."""
    out = []
    for name in layouts:
        if name == "fresh":
            continue
        for slot in range(3):
            out.append(tuple(name if k == slot else "fresh" for k in range(3)))
        out.append((name,) * 3)
    if broadcast:
        out += [("fresh", "broadcast", "fresh"), ("fresh", "fresh", "broadcast"), ("fresh", "broadcast", "broadcast")]
    return out


# the shapes of tests/test_field_layouts_gpu.py: H*W odd everywhere (``tail`` and the per-map bases misalign), B = 3
B = 3
EXACT_SHAPES = ((5, 7), (33, 33), (65, 65))      # the 64-, 256- and 1024-lane workgroups of the exact one-workgroup kernels
TILED_SHAPES = ((65, 65), (1, 197))              # 2x2 tiles, ragged both ways; one row
SOFT_SHAPES = ((5, 7), (31, 33))                 # of soft_fields_oracle.SHAPE_CASES
SOFT_TILED_SHAPES = ((65, 65),)                  # horizon 24, checkpoint_every 5: a partial last segment
MASKS = (0x1EF, 0x0EB)                           # Moore-8 and a directed move set
