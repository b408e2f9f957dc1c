"""GPU tests (-m gpu): the solvability proof runs on a side stream BESIDE the search, ordered behind the caller's stream by an event that
carries no system-scope fence (csrc/nastar_verdict_capi.hip: hipEventDisableSystemFence -- the marker between two search launches is a
plain barrier).  What that event must still guarantee: the proof sees what the caller's stream wrote into the maps just before the call.

Here the maps are REWRITTEN IN PLACE on the caller's stream -- a copy kernel, 16 MB, no synchronisation of ours -- directly in front of
every proof launch, alternating between a batch of solvable maps and the same batch with some goals walled in.  A proof that started early,
or read stale lines, would report the previous content."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


def _variants(B, W):
    """(solvable maps, the same with the goals of a few maps walled in, starts, goals) as device tensors [B, W, W]"""
    from neural_astar.utils import synthetic as syn
    pr = syn.maze_maps(64, W, seed=17)
    pick = np.random.default_rng(3).integers(64, size=B)
    m, s, g = (np.ascontiguousarray(x[pick, 0]) for x in pr)
    bad = m.copy()
    for b in (0, 7, B // 2, B - 1):
        gy, gx = divmod(int(g[b].reshape(-1).argmax()), W)
        bad[b, max(gy - 1, 0):gy + 2, max(gx - 1, 0):gx + 2] = 0
        bad[b, gy, gx] = 1
    return tuple(torch.from_numpy(x).to(_dev()) for x in (m, bad, s, g))


def _prove(lib, buf, s, g, proved, word_ptr, counter_ptr):
    B, W = buf.shape[0], buf.shape[-1]
    rc = lib.nastar_solvable_proof(buf.data_ptr(), s.data_ptr(), g.data_ptr(), buf.data_ptr(), B, W, W, proved.data_ptr(), word_ptr, counter_ptr,
                                   torch.cuda.current_stream(_dev()).cuda_stream)
    assert rc == 0


@pytest.mark.parametrize("W", [32, 64])
def test_the_proof_sees_maps_the_stream_wrote_just_before(W):
    from neural_astar import _native
    lib = _native.load()
    dev = _dev()
    B = 4096 if W == 32 else 1024
    good, bad, s, g = _variants(B, W)
    buf = torch.empty_like(good)
    n = 24
    words = torch.zeros((n + 2, 16), dtype=torch.int32).pin_memory()
    counters = torch.zeros(n + 2, dtype=torch.int32, device=dev)
    # what each variant gives when everything around the launch is synchronised
    ref = {}
    for k, (name, src) in enumerate((("good", good), ("bad", bad))):
        buf.copy_(src)
        torch.cuda.synchronize()
        proved = torch.full((B,), -1, dtype=torch.int32, device=dev)
        _prove(lib, buf, s, g, proved, words[n + k].data_ptr(), counters[n + k:].data_ptr())
        assert lib.nastar_solvable_proof_sync() == 0
        ref[name] = (proved.cpu().numpy(), int(words[n + k, 0]))
    assert ref["good"][1] != ref["bad"][1] and not np.array_equal(ref["good"][0], ref["bad"][0])
    # the same, back to back: rewrite in place, launch, no synchronisation in between
    order = np.random.default_rng(11).integers(2, size=n)
    order[:4] = (0, 1, 0, 1)
    outs = []
    for k in range(n):
        buf.copy_(bad if order[k] else good)   # on the caller's stream, right in front of the proof's event
        proved = torch.full((B,), -1, dtype=torch.int32, device=dev)
        _prove(lib, buf, s, g, proved, words[k].data_ptr(), counters[k:].data_ptr())
        # the NEXT rewrite of `buf` must not overtake this proof: the host waits for the side stream (the copy in front of the launch was
        # NOT waited for -- only the event orders the proof behind it)
        assert lib.nastar_solvable_proof_sync() == 0
        outs.append(proved)
    torch.cuda.synchronize()
    for k in range(n):
        want = ref["bad" if order[k] else "good"]
        assert int(words[k, 0]) == want[1], f"launch {k} ({'bad' if order[k] else 'good'} maps): word {int(words[k, 0])}"
        assert np.array_equal(outs[k].cpu().numpy(), want[0]), f"launch {k}: proved[] differs from the synchronised launch"


def test_forward_raises_for_maps_written_just_before_the_call():
    """the whole path: VanillaAstar.forward() on a buffer the stream rewrote in place a moment earlier -- the early verdict (the proof's) must
    be the one of the NEW content, call after call"""
    from neural_astar.planner import VanillaAstar
    from neural_astar.planner.differentiable_astar import UnsolvableMapError
    good, bad, s, g = _variants(4096, 32)
    buf = torch.empty_like(good)[:, None]
    va = VanillaAstar().to(_dev()).eval()
    order = np.random.default_rng(5).integers(2, size=30)
    order[:4] = (0, 1, 0, 1)
    with torch.no_grad():
        ref = va(good[:, None], s[:, None], g[:, None])
        for k in range(30):
            buf.copy_((bad if order[k] else good)[:, None])
            if order[k]:
                with pytest.raises(UnsolvableMapError):
                    va(buf, s[:, None], g[:, None])
            else:
                out = va(buf, s[:, None], g[:, None])
                if k % 8 == 0:
                    assert torch.equal(out.paths, ref.paths)
