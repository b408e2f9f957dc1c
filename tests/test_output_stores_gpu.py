"""GPU tests (-m gpu) of how the forward search kernels STORE their outputs: compact_store_hist / compact_store_outputs
(csrc/nastar_search_compact.hip.h), unit_store_hist / unit_store_paths (csrc/nastar_search_unit.hip.h) and the large-map kernels' loops.

Aligned outputs of maps whose width is a multiple of 4 are written 16 bytes per lane, one kilobyte per wave instruction; everything else
takes element-wise fall-back loops.  Written while those 16-byte loops were tried as write-through stores through one buffer resource per
map row (measured and dropped: NOTES.md, profiles/writethrough_outputs.json); the tests hold for any flavour of store.  What can go wrong
in such a loop is a row's base, a row's size, an offset, or a consumer reading a stale line -- so every test compares with the CPU oracle:

  * bit-exact histories, paths, iters and status at the store loops' edge shapes (one lane-iteration, several, a partial one; one map, three,
    65 -- two blocks of the ranked placement, one of them partial, and workgroups that return without a map), for every kernel family;
  * unaligned outputs through the C ABI take the fall-back loops and still equal the oracle;
  * guard bytes around the outputs stay untouched;
  * outputs are visible to a consumer on the same stream, on a second stream behind an event, and to the host, without any fence of ours.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 8192  # bytes in front of and behind every carved output (the issue asks for at least 4 KB)
SENTINEL = 0xA5


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


@functools.lru_cache(maxsize=None)
def _case(H, W, B, mask=None):
    """(problems, oracle outputs) of one seeded batch: computed once, shared by every test that needs it, never modified"""
    from neural_astar.utils import synthetic as syn
    from oracle import oracle as O
    pr = syn.random_obstacle_maps(B, H, W, 0.2, seed=1000 * H + W + B)
    o = O.forward(pr.map_designs, pr.start_maps, pr.goal_maps, pr.map_designs, 0.5, H * W, mode="sm",
                  **({} if mask is None else {"neighbor_mask": mask}))
    for a in (o.histories, o.paths, o.iters, o.map_status):
        a.setflags(write=False)
    return pr, o


def _levels(pr):
    """|opt_dist[start]| as a data set carries it (what ops.attach_levels expects)"""
    from neural_astar.utils import synthetic as syn
    B = pr.map_designs.shape[0]
    gi = pr.goal_maps.reshape(B, -1).argmax(1)
    si = pr.start_maps.reshape(B, -1).argmax(1)
    d = syn.geodesic_distance(pr.map_designs[:, 0] > 0, gi).reshape(B, -1)
    return d[np.arange(B), si].astype(np.int32)


def _assert_oracle(o, hist, paths, iters, status, what):
    hist, paths, iters, status = (x.cpu().numpy() for x in (hist, paths, iters, status))
    assert np.array_equal(hist.reshape(o.histories.shape).view(np.uint32), o.histories.view(np.uint32)), f"{what}: histories"
    assert np.array_equal(paths.reshape(o.paths.shape), o.paths), f"{what}: paths"
    assert np.array_equal(iters, o.iters), f"{what}: iters"
    assert np.array_equal(status, o.map_status), f"{what}: status"


def _op(pr, flags=0, mask=None):
    """one launch through the custom op: cost and passable are ONE tensor (VanillaAstar's call)"""
    from neural_astar import ops
    m, s, g = (_t(x[:, 0]) for x in pr)
    H, W = m.shape[1:]
    out = torch.ops.nastar.astar_forward(m, s, g, m, 0.5, H * W, False, int(flags), 0, False, ops.NEIGHBORS_MOORE8 if mask is None else int(mask))
    torch.cuda.synchronize()
    return out[:4]


# ---- bit-exact outputs at the store loops' edge shapes --------------------------------------------------------------------------------------

# 16x16: 64 float4 per row = ONE lane-iteration of the histories loop, two of the paths loop; 32x32: four and eight; 64x64: sixteen and 32
@pytest.mark.parametrize("B", [1, 3, 65])
@pytest.mark.parametrize("H", [16, 32, 64])
def test_hand_scheduled_family_equals_the_oracle(H, B):
    pr, o = _case(H, H, B)
    _assert_oracle(o, *_op(pr), f"{H}x{H} B={B}")


@pytest.mark.parametrize("B", [1, 3, 65])
@pytest.mark.parametrize("H", [16, 32, 64])
def test_ranked_placement_equals_the_oracle(H, B):
    """levels attached to the start maps: the launch places the maps itself (nastar_forward_compact_ranked_kernel).  B = 65: two blocks of
    ranks, the second one partial, and 63 workgroups that find no map and return before any store."""
    from neural_astar import ops
    from neural_astar.planner import VanillaAstar
    pr, o = _case(H, H, B)
    m, s, g = (_t(x) for x in pr)
    ops.attach_levels(s, _t(_levels(pr)))
    va = VanillaAstar().to(_dev()).eval()
    with torch.no_grad():
        out = va(m, s, g)
    torch.cuda.synchronize()
    _assert_oracle(o, out.histories, out.paths, va.astar.last_iters, va.astar.last_status, f"ranked {H}x{H} B={B}")


@pytest.mark.parametrize("B", [1, 3, 65])
@pytest.mark.parametrize("H", [32, 64])
def test_unit_cost_kernel_equals_the_oracle(H, B):
    from neural_astar import ops
    pr, o = _case(H, H, B)
    _assert_oracle(o, *_op(pr, flags=ops.FLAG_UNIT_COST), f"unit-cost {H}x{H} B={B}")


@pytest.mark.parametrize("H,W,B", [(20, 45, 1), (20, 45, 3), (20, 45, 65),   # W % 4 != 0: the compiled kernel's element-wise stores
                                   (20, 44, 3), (20, 44, 65),                 # 220 float4 per row: the 16-byte loops with a partial last iteration
                                   (96, 96, 3), (150, 150, 2)])               # the large-map kernels (state beyond LDS: HBM slab)
def test_compiled_and_large_map_kernels_equal_the_oracle(H, W, B):
    pr, o = _case(H, W, B)
    _assert_oracle(o, *_op(pr), f"{H}x{W} B={B}")


@pytest.mark.parametrize("H,W,B", [(32, 32, 65), (20, 44, 3)])
def test_masked_neighbourhood_equals_the_masked_oracle(H, W, B):
    """a neighbor_filter call (4-connected): the masked twins of the kernels share the store loops"""
    from neural_astar import ops
    pr, o = _case(H, W, B, ops.NEIGHBORS_VON_NEUMANN)
    _assert_oracle(o, *_op(pr, mask=ops.NEIGHBORS_VON_NEUMANN), f"von Neumann {H}x{W} B={B}")


# ---- raw C ABI on carved buffers: unaligned outputs, guard bytes --------------------------------------------------------------------------

def _raw_launch(pr, shift_h, shift_p):
    """nastar_forward_ex with histories / paths carved out of sentinel-filled byte buffers, `shift` bytes past a 4 KB-aligned GUARD.
    -> (hist bytes, paths bytes, iters, status) with the guards still around the two outputs"""
    from neural_astar import _native
    lib = _native.load()
    dev = _dev()
    m, s, g = (_t(x[:, 0]) for x in pr)
    B, H, W = m.shape
    nh, npth = B * H * W * 4, B * H * W * 8
    bh = torch.full((GUARD + shift_h + nh + GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
    bp = torch.full((GUARD + shift_p + npth + GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
    assert bh.data_ptr() % 16 == 0 and bp.data_ptr() % 16 == 0
    it = torch.empty(B, dtype=torch.int32, device=dev)
    st = torch.empty(B, dtype=torch.int32, device=dev)
    rc = lib.nastar_forward_ex(m.data_ptr(), s.data_ptr(), g.data_ptr(), m.data_ptr(), B, H, W, 0.5, H * W,
                               bh.data_ptr() + GUARD + shift_h, bp.data_ptr() + GUARD + shift_p, None,
                               it.data_ptr(), st.data_ptr(), None, None, 0, 0, None, None, None, None, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return bh.cpu().numpy(), bp.cpu().numpy(), it, st


def _check_carved(o, raw, shift_h, shift_p, what):
    bh, bp, it, st = raw
    nh, npth = o.histories.size * 4, o.paths.size * 8
    for name, buf, lo, n in (("histories", bh, GUARD + shift_h, nh), ("paths", bp, GUARD + shift_p, npth)):
        assert (buf[:lo] == SENTINEL).all(), f"{what}: bytes in FRONT of {name} were written"
        assert (buf[lo + n:] == SENTINEL).all(), f"{what}: bytes BEHIND {name} were written"
    hist = np.frombuffer(bh[GUARD + shift_h:GUARD + shift_h + nh].tobytes(), np.uint32).reshape(o.histories.shape)
    paths = np.frombuffer(bp[GUARD + shift_p:GUARD + shift_p + npth].tobytes(), np.int64).reshape(o.paths.shape)
    assert np.array_equal(hist, o.histories.view(np.uint32)), f"{what}: histories"
    assert np.array_equal(paths, o.paths), f"{what}: paths"
    assert np.array_equal(it.cpu().numpy(), o.iters) and np.array_equal(st.cpu().numpy(), o.map_status), f"{what}: iters / status"


@pytest.mark.parametrize("B", [1, 65])
@pytest.mark.parametrize("H", [32, 64])
def test_guard_bytes_around_the_outputs_stay_untouched(H, B):
    """a wrong row size or offset would write (or leave out) bytes at a row's edge: every guard byte keeps the sentinel"""
    pr, o = _case(H, H, B)
    _check_carved(o, _raw_launch(pr, 0, 0), 0, 0, f"{H}x{H} B={B}")


@pytest.mark.parametrize("shift_h,shift_p", [(4, 8), (8, 4), (4, 0), (0, 8)])
@pytest.mark.parametrize("H,W,B", [(32, 32, 3), (32, 32, 65), (20, 45, 3)])
def test_unaligned_outputs_take_the_fall_back_stores(H, W, B, shift_h, shift_p):
    """histories / paths 4 or 8 bytes off a 16-byte boundary: the launch must take the element-wise loops (a 16-byte store there would be
    misplaced or torn), equal the oracle and leave the guards alone"""
    pr, o = _case(H, W, B)
    _check_carved(o, _raw_launch(pr, shift_h, shift_p), shift_h, shift_p, f"{H}x{W} B={B} +{shift_h}/+{shift_p}")


# ---- visibility without a fence -------------------------------------------------------------------------------------------------------------

def _sums(o):
    return int(o.histories.astype(np.float64).sum()), int(o.paths.sum()), o.histories.sum((1, 2)).astype(np.int64), o.paths.sum((1, 2))


def _launch(pr):
    from neural_astar import ops
    m, s, g = (_t(x) for x in pr)
    torch.cuda.synchronize()
    H, W = m.shape[2:]
    return ops.search_nograd(m, s, g, m, 0.5, H * W)[:2]  # returns while the launch runs: nothing here waits for the device


@pytest.mark.parametrize("H,B", [(32, 512), (64, 65)])
def test_outputs_are_visible_to_a_reduction_on_the_same_stream(H, B):
    pr, o = _case(H, H, B)
    hist, paths = _launch(pr)
    hs, ps = hist.sum((1, 2), dtype=torch.float64), paths.sum((1, 2))  # queued right behind the launch
    th, tp, rh, rp = _sums(o)
    assert np.array_equal(hs.cpu().numpy().astype(np.int64), rh) and np.array_equal(ps.cpu().numpy(), rp)
    assert int(hs.sum()) == th and int(ps.sum()) == tp


@pytest.mark.parametrize("H,B", [(32, 512), (64, 65)])
def test_outputs_are_visible_on_a_second_stream_behind_an_event(H, B):
    pr, o = _case(H, H, B)
    side = torch.cuda.Stream(_dev())
    hist, paths = _launch(pr)
    ev = torch.cuda.Event()
    ev.record()
    with torch.cuda.stream(side):
        side.wait_event(ev)
        hs, ps = hist.sum((1, 2), dtype=torch.float64), paths.sum((1, 2))
    side.synchronize()
    torch.cuda.synchronize()
    th, tp, rh, rp = _sums(o)
    assert np.array_equal(hs.cpu().numpy().astype(np.int64), rh) and np.array_equal(ps.cpu().numpy(), rp)


@pytest.mark.parametrize("H,B", [(32, 512), (64, 65)])
def test_outputs_are_visible_to_a_host_copy_after_synchronize(H, B):
    pr, o = _case(H, H, B)
    hist, paths = _launch(pr)
    torch.cuda.synchronize()
    h, p = hist.cpu().numpy(), paths.cpu().numpy()
    assert np.array_equal(h.reshape(o.histories.shape), o.histories) and np.array_equal(p.reshape(o.paths.shape), o.paths)
