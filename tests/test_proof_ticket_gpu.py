"""GPU tests (-m gpu) of include/nastar_ticket.h: nastar_forward_proved issues a search launch and the proof of its batch from one call, and
orders the proof behind the search launch's own START (a ticket that workgroup 0 stores, a stream memory wait on the side stream) instead of
an event in front of the launch.

  1. same verdicts: the entry point == nastar_solvable_proof + nastar_forward_ex / nastar_forward_levels, bit for bit, in the ticket order
     and (a child process under NASTAR_PROOF_ORDER=event) in the event order
  2. order against producers: maps rewritten in place on the caller's stream in front of every call
  3. the ring of tickets is reused; 4. two caller streams; 5. a refused search launch leaves nothing pending; 6. through forward()

A wait that is never satisfied would show as a hang of nastar_solvable_proof_sync(): run this file under a time limit.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import proof_ticket_cases as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RING = 32  # NASTAR_TICKET_RING


def _lib():
    from neural_astar import _native
    return _native.load()


def _ticket(lib):
    """the ticket order is what the device these tests run on MUST get: signal memory, stream memory waits, the ring.  Only a process started
    with NASTAR_PROOF_ORDER=event may see the event order; a library that quietly fell back to it fails here, in every test of this file."""
    forced = os.environ.get("NASTAR_PROOF_ORDER") == "event"
    assert lib.nastar_proof_ticket_available() == (0 if forced else 1), "the ticket order is not available on this device"
    return not forced


def test_the_ticket_order_is_taken_on_this_device():
    lib = _lib()
    assert _ticket(lib) or os.environ.get("NASTAR_PROOF_ORDER") == "event"
    good, _, s, g, _ = _two_contents(3)
    before = C.order_counts(lib)
    assert C.call_proved(lib, good, s, g, C.Out(3, 32)) == (0, 0)
    C.finish(lib)
    after = C.order_counts(lib)
    assert (after[0] - before[0], after[1] - before[1]) == ((1, 0) if _ticket(lib) else (0, 1))


def test_the_header_constant_is_the_ring_of_this_file():
    hdr = open(os.path.join(ROOT, "include", "nastar_ticket.h")).read()
    assert f"#define NASTAR_TICKET_RING {RING} " in hdr


# ---- 1. same verdicts --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,W", C.SHAPES)
@pytest.mark.parametrize("levels", [False, True], ids=["forward_ex", "forward_levels"])
def test_same_verdicts_as_the_two_calls(B, W, levels):
    lib = _lib()
    C.check_same_verdicts(lib, B, W, levels, want_ticket=_ticket(lib))


def test_forced_event_order_gives_the_same_verdicts():
    """NASTAR_PROOF_ORDER=event is read once in native code: a process of its own"""
    env = dict(os.environ, NASTAR_PROOF_ORDER="event")
    code = ("import sys; sys.path[:0] = [%r, %r, %r]; import proof_ticket_cases as C; C.main_event_order()"
            % (os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "neural-astar_amd")))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "event order ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- 2. order against producers ------------------------------------------------------------------------------------------------------------
def _two_contents(B, W=32):
    """(solvable maps, the same with every fourth goal walled in, starts, goals) on the device, and what a synchronised proof says of each"""
    lib = _lib()
    pm, ps, pg = C.pool(W)
    pick = np.random.default_rng(23).integers(pm.shape[0], size=B)
    good, s, g = pm[pick].copy(), ps[pick].copy(), pg[pick].copy()
    bad = good.copy()
    for b in range(0, B, 4):
        gy, gx = divmod(int(g[b].reshape(-1).argmax()), W)
        bad[b, max(gy - 1, 0):gy + 2, max(gx - 1, 0):gx + 2] = 0
        bad[b, gy, gx] = 1
    want = {0: (C.flood_proved(good, s, g), None), 1: (C.flood_proved(bad, s, g), None)}
    assert want[0][0].all() and not want[1][0][0] and (B < 2 or want[1][0][1])
    good, bad, s, g = C.t(good), C.t(bad), C.t(s), C.t(g)
    ref = {}
    for k, src in ((0, good), (1, bad)):
        out = C.Out(B, W)
        assert C.call_pair(lib, src, s, g, out) == (0, 0)
        C.finish(lib)
        a = out.arrays()
        assert np.array_equal(a["proved"], want[k][0]) and int(a["word"]) == (2 if k else 1)
        ref[k] = a
    return good, bad, s, g, ref


@pytest.mark.parametrize("B", [2, 130])
def test_every_call_sees_the_maps_written_just_before_it(B):
    """64 consecutive calls; in front of each the caller's stream overwrites the maps in place with solvable or unsolvable contents, by a
    seeded pattern.  Nothing but the order of the caller's stream keeps a proof from reading the previous contents.  Four buffers take
    turns, and the host looks at the word of the call four back before it lets a buffer be overwritten again (the proof that read it must be
    over -- by then it long is): the queue stays full, and no stream is ever waited for."""
    lib = _lib()
    good, bad, s, g, ref = _two_contents(B)
    n, nbuf = 64, 4
    bufs = [torch.empty_like(good) for _ in range(nbuf)]
    pattern = np.random.default_rng(11).integers(2, size=n)
    pattern[:4] = (0, 1, 0, 1)
    outs = [C.Out(B, 32) for _ in range(n)]
    before = C.order_counts(lib)
    for k in range(n):
        if k >= nbuf:
            assert lib.nastar_host_wait_nonzero(outs[k - nbuf].word.data_ptr(), 5_000_000) == 1, f"the proof of call {k - nbuf} did not end"
        buf = bufs[k % nbuf]
        buf.copy_(bad if pattern[k] else good)
        assert C.call_proved(lib, buf, s, g, outs[k]) == (0, 0)
    C.finish(lib)
    after = C.order_counts(lib)
    # every one of them by ticket: the host has seen the word of call k - 4, so the half ring that call k may enter is free -- each slot is
    # used twice here, the second time by ticket
    assert (after[0] - before[0], after[1] - before[1]) == ((n, 0) if _ticket(lib) else (0, n))
    for k in range(n):
        a, want = outs[k].arrays(), ref[int(pattern[k])]
        assert int(a["word"]) == int(want["word"]), f"call {k} ({'bad' if pattern[k] else 'good'} maps): word {int(a['word'])}"
        for key in want:
            assert np.array_equal(a[key], want[key]), f"call {k}: {key} is not that of the contents written for it"


# ---- 3. ring reuse -----------------------------------------------------------------------------------------------------------------------
def test_more_calls_than_the_ring_has_slots_before_the_first_wait():
    """RING + 3 calls with no host wait.  The searches run one after another on the caller's stream and the host is far ahead of them, so the
    first ticket of a half ring that was handed out in THIS burst usually finds that half's proofs still pending and the call falls back to
    the event order, as do the calls behind it until the half is free.  What is certain: the rest of the half the burst starts in (at least
    one ticket) and the whole other half (RING / 2 tickets; its earlier proofs ended before the burst) go by ticket.  Every call, by ticket or
    by event, must give a terminal and right word.  (Reuse of every slot BY TICKET under a full queue:
    test_every_call_sees_the_maps_written_just_before_it.)"""
    lib = _lib()
    good, bad, s, g, ref = _two_contents(3)
    n = RING + 3
    outs = [C.Out(3, 32) for _ in range(n)]
    before = C.order_counts(lib)
    for k in range(n):  # back to back at the C ABI: no host wait, nothing rewritten
        assert C.call_proved(lib, bad if k % 3 == 1 else good, s, g, outs[k]) == (0, 0)
    C.finish(lib)
    after = C.order_counts(lib)
    by_ticket, by_event = after[0] - before[0], after[1] - before[1]
    print(f"{n} calls back to back: {by_ticket} by ticket, {by_event} by event")
    assert by_ticket + by_event == n
    assert by_ticket >= RING // 2 + 1 if _ticket(lib) else by_ticket == 0
    for k in range(n):
        a, want = outs[k].arrays(), ref[1 if k % 3 == 1 else 0]
        for key in want:
            assert np.array_equal(a[key], want[key]), (k, key)


# ---- 4. two caller streams -----------------------------------------------------------------------------------------------------------------
def test_two_caller_streams_interleave():
    lib = _lib()
    good, bad, s, g, ref = _two_contents(130)
    streams = [torch.cuda.Stream(C.dev()), torch.cuda.Stream(C.dev())]
    torch.cuda.synchronize()
    n = 12
    outs = [C.Out(130, 32) for _ in range(n)]
    torch.cuda.synchronize()  # (the outputs were filled on the current stream)
    for k in range(n):
        assert C.call_proved(lib, bad if k % 2 else good, s, g, outs[k], stream=streams[k % 2]) == (0, 0)
    assert lib.nastar_solvable_proof_sync() == 0
    torch.cuda.synchronize()
    for k in range(n):
        a, want = outs[k].arrays(), ref[k % 2]
        for key in want:
            assert np.array_equal(a[key], want[key]), (k, key)


# ---- 5. a refused search launch --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("over,rc", [(dict(max_iters=0), 1), (dict(flags=1 << 20), 2)], ids=["bad_shape", "unknown_flag"])
def test_a_refused_search_launch_leaves_no_proof_pending(over, rc):
    lib = _lib()
    good, _, s, g, ref = _two_contents(3)
    out = C.Out(3, 32)
    torch.cuda.synchronize()
    got_rc, prc = C.call_proved(lib, good, s, g, out, **over)
    assert got_rc == rc and prc != 0
    assert lib.nastar_solvable_proof_sync() == 0  # (returns: nothing waits for a ticket that no launch will store)
    torch.cuda.synchronize()
    assert int(out.word[0]) == 0 and int(out.counter.cpu()[0]) == 0 and (out.proved.cpu().numpy() == -7).all()
    # and the next call is served as usual
    out2 = C.Out(3, 32)
    assert C.call_proved(lib, good, s, g, out2) == (0, 0)
    C.finish(lib)
    for key, v in ref[0].items():
        assert np.array_equal(out2.arrays()[key], v), key


# ---- 6. through the API ----------------------------------------------------------------------------------------------------------------------
def test_forward_takes_the_entry_point():
    """forward() returns on the proof, and the native host lane issues search and proof from the one entry point, for a batch of 5 and a batch of 512 maps"""
    from neural_astar.planner import VanillaAstar
    from neural_astar.planner.differentiable_astar import UnsolvableMapError
    lib = _lib()
    good, bad, s, g, ref = _two_contents(5)
    va = VanillaAstar().to(C.dev()).eval()
    with torch.no_grad():
        before = C.order_counts(lib)
        out = va(good[:, None], s[:, None], g[:, None])
        assert va.astar.last_verdict_source == "proof"
        torch.cuda.synchronize()
        assert np.array_equal(out.histories[:, 0].cpu().numpy(), ref[0]["hist"]) and np.array_equal(out.paths[:, 0].cpu().numpy(), ref[0]["paths"])
        with pytest.raises(UnsolvableMapError):
            va(bad[:, None], s[:, None], g[:, None])
        after = C.order_counts(lib)
        assert (after[0] - before[0], after[1] - before[1]) == ((2, 0) if _ticket(lib) else (0, 2))
        rep = lambda x, n: x.repeat(103, 1, 1)[:n, None].contiguous()  # noqa: E731 -- the five maps over and over
        n = 512  # (more than one pass of the proof's grid)
        before = C.order_counts(lib)
        out = va(rep(good, n), rep(s, n), rep(g, n))
        assert va.astar.last_verdict_source == "proof"
        after = C.order_counts(lib)
        assert (after[0] - before[0], after[1] - before[1]) == ((1, 0) if _ticket(lib) else (0, 1)), n
        torch.cuda.synchronize()
        assert np.array_equal(out.histories[:5, 0].cpu().numpy(), ref[0]["hist"]) and np.array_equal(out.paths[505:510, 0].cpu().numpy(), ref[0]["paths"])
        before = after
        with pytest.raises(UnsolvableMapError):
            va(rep(bad, n), rep(s, n), rep(g, n))
        assert sum(C.order_counts(lib)) - sum(before) == 1
