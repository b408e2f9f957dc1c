"""Shared by tests/test_proof_ticket_gpu.py and the child process it starts under NASTAR_PROOF_ORDER=event: batches that mix the cases of
include/nastar_verdict.h, one call of nastar_forward_proved (include/nastar_ticket.h), and the same work as the two calls it replaces."""
import ctypes
import functools

import numpy as np
import torch

KINDS = ("solvable", "walled_goal", "no_start", "cost_above_bound", "start_is_goal")
# one above bound (b) of include/nastar_verdict.h: 61440 / (H * W) is 60 on a 32x32 map and 15 on a 64x64 map
OVER = {32: 61.0, 64: 16.0}


def dev():
    assert torch.cuda.is_available(), "needs a HIP device"
    return torch.device("cuda:0")


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


@functools.lru_cache(maxsize=None)
def pool(W):
    from neural_astar.utils import synthetic as syn
    return tuple(np.ascontiguousarray(x[:, 0]) for x in syn.maze_maps(64, W, seed=17))


def mixed_batch(B, W, shift=0, seed=3):
    """(maps, starts, goals) as numpy [B, W, W] fp32 and the kind of every map: map b is of kind KINDS[(b + shift) % 5].  The maps serve as
    cost AND passable (one tensor), so the cost above the bound sits on a passable cell."""
    pm, ps, pg = pool(W)
    pick = np.random.default_rng(seed + 7 * B + shift).integers(pm.shape[0], size=B)
    m, s, g = pm[pick].copy(), ps[pick].copy(), pg[pick].copy()
    kinds = [KINDS[(b + shift) % len(KINDS)] for b in range(B)]
    for b, kind in enumerate(kinds):
        gy, gx = divmod(int(g[b].reshape(-1).argmax()), W)
        if kind == "walled_goal":
            m[b, max(gy - 1, 0):gy + 2, max(gx - 1, 0):gx + 2] = 0
            m[b, gy, gx] = 1
        elif kind == "no_start":
            s[b] = 0
        elif kind == "cost_above_bound":
            m[b, gy, gx] = OVER[W]
        elif kind == "start_is_goal":
            s[b] = g[b]
    return m, s, g, kinds


def flood_proved(m, s, g):
    """proved[] by the rule of include/nastar_verdict.h, in numpy: start and goal exist, every cost within [0, 61440 / (H * W)], the goal in the
    8-neighbour closure of the start over the non-zero cells"""
    B, H, W = m.shape
    out = np.zeros(B, dtype=np.int32)
    for b in range(B):
        if not s[b].any() or not g[b].any() or not ((m[b] >= 0) & (m[b] <= 61440.0 / (H * W))).all():
            continue
        si, gi = np.flatnonzero(s[b].reshape(-1)).max(), np.flatnonzero(g[b].reshape(-1)).max()
        seen = np.zeros((H + 2, W + 2), dtype=bool)
        seen[si // W + 1, si % W + 1] = True
        ok = np.zeros((H + 2, W + 2), dtype=bool)
        ok[1:-1, 1:-1] = m[b] != 0
        while True:
            grow = np.zeros_like(seen)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    grow |= np.roll(np.roll(seen, dy, 0), dx, 1)
            grow = (grow & ok) | seen
            if (grow == seen).all():
                break
            seen = grow
        out[b] = int(seen[gi // W + 1, gi % W + 1])
    return out


class Out:
    """the outputs of one call: the search's four arrays, proved[], and the proof's status row (word in pinned memory, counter on the device)"""

    def __init__(self, B, W):
        d = dev()
        self.hist = torch.full((B, W, W), -7.0, dtype=torch.float32, device=d)
        self.paths = torch.full((B, W, W), -7, dtype=torch.int64, device=d)
        self.iters = torch.full((B,), -7, dtype=torch.int32, device=d)
        self.status = torch.full((B,), -7, dtype=torch.int32, device=d)
        self.proved = torch.full((B,), -7, dtype=torch.int32, device=d)
        self.word = torch.zeros(16, dtype=torch.int32).pin_memory()
        self.counter = torch.zeros(1, dtype=torch.int32, device=d)

    def arrays(self):
        return {k: getattr(self, k).cpu().numpy() for k in ("hist", "paths", "iters", "status", "proved")} | {"word": np.array(int(self.word[0]))}


def _stream(stream):
    return (torch.cuda.current_stream(dev()) if stream is None else stream).cuda_stream


def call_proved(lib, m, s, g, out, levels=None, stream=None, max_iters=None, flags=0):
    """nastar_forward_proved -> (rc of the search launch, rc of the proof)"""
    B, W = m.shape[0], m.shape[-1]
    prc = ctypes.c_int(-99)
    rc = lib.nastar_forward_proved(m.data_ptr(), s.data_ptr(), g.data_ptr(), m.data_ptr(), B, W, W, 0.5, W * W if max_iters is None else max_iters,
                                   out.hist.data_ptr(), out.paths.data_ptr(), None, out.iters.data_ptr(), out.status.data_ptr(), None, None, 0, flags,
                                   None, None, None, None, None if levels is None else levels.data_ptr(), out.proved.data_ptr(),
                                   out.word.data_ptr(), out.counter.data_ptr(), ctypes.addressof(prc), _stream(stream))
    return rc, prc.value


def call_pair(lib, m, s, g, out, levels=None, stream=None):
    """the two calls nastar_forward_proved replaces: nastar_solvable_proof, then nastar_forward_ex / nastar_forward_levels"""
    B, W = m.shape[0], m.shape[-1]
    st = _stream(stream)
    prc = lib.nastar_solvable_proof(m.data_ptr(), s.data_ptr(), g.data_ptr(), m.data_ptr(), B, W, W, out.proved.data_ptr(), out.word.data_ptr(),
                                    out.counter.data_ptr(), st)
    head = (m.data_ptr(), s.data_ptr(), g.data_ptr(), m.data_ptr(), B, W, W, 0.5, W * W, out.hist.data_ptr(), out.paths.data_ptr(), None,
            out.iters.data_ptr(), out.status.data_ptr(), None, None, 0, 0)
    if levels is None:
        rc = lib.nastar_forward_ex(*head, None, None, None, None, st)
    else:
        rc = lib.nastar_forward_levels(*head, levels.data_ptr(), None, None, st)
    return rc, prc


def order_counts(lib):
    a, b = ctypes.c_longlong(-1), ctypes.c_longlong(-1)
    assert lib.nastar_proof_order_counts(ctypes.addressof(a), ctypes.addressof(b)) == 0
    return a.value, b.value


def finish(lib):
    assert lib.nastar_solvable_proof_sync() == 0
    torch.cuda.synchronize()


SHAPES = [(1, 32), (2, 32), (3, 32), (129, 32), (1, 64), (3, 64)]


def check_same_verdicts(lib, B, W, use_levels, want_ticket):
    """nastar_forward_proved == nastar_solvable_proof + nastar_forward_ex / _levels, bit for bit, on mixed batches; the proofs were ordered
    the way `want_ticket` says.  Small batches rotate the kinds so that every kind is seen at every position."""
    for shift in (range(len(KINDS)) if B < len(KINDS) else (0,)):
        m, s, g, kinds = (mixed_batch(B, W, shift))
        m, s, g = t(m), t(s), t(g)
        levels = t(np.random.default_rng(5 + shift).integers(0, 200, size=B).astype(np.int32)) if use_levels else None
        ref, got = Out(B, W), Out(B, W)
        assert call_pair(lib, m, s, g, ref, levels) == (0, 0)
        finish(lib)
        before = order_counts(lib)
        assert call_proved(lib, m, s, g, got, levels) == (0, 0)
        finish(lib)
        after = order_counts(lib)
        assert (after[0] - before[0], after[1] - before[1]) == ((1, 0) if want_ticket else (0, 1)), (before, after)
        a, b = ref.arrays(), got.arrays()
        assert int(a["word"]) in (1, 2)
        for k in a:
            assert np.array_equal(a[k], b[k]), (k, B, W, shift, kinds)
        want = flood_proved(m.cpu().numpy(), s.cpu().numpy(), g.cpu().numpy())
        for b_, kind in enumerate(kinds):  # (the kinds are what they claim to be)
            assert want[b_] == (kind in ("solvable", "start_is_goal")), (b_, kind)
        assert np.array_equal(b["proved"], want), (kinds, b["proved"])
        assert int(b["word"]) == (1 if want.all() else 2)


def main_event_order():
    """run by the child process of test_forced_event_order_gives_the_same_verdicts, with NASTAR_PROOF_ORDER=event in its environment"""
    from neural_astar import _native
    lib = _native.load()
    assert lib.nastar_proof_ticket_available() == 0
    for B, W in SHAPES:
        check_same_verdicts(lib, B, W, use_levels=(B == 129), want_ticket=False)
    assert order_counts(lib)[0] == 0
    print("event order ok")
