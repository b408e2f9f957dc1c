"""CPU: include/nastar_ticket.h (a search launch and the proof of its batch from one call) -- everything that needs no GPU.

1. the sixteenth header against ``_native.TICKET_SIGNATURES``; the library exports and binds its symbols; the three headers it stands beside
   do not name it;
2. the one refusal made before any HIP call;
3. the batches of the GPU tests are what they claim to be (tests/proof_ticket_cases.py).
"""
import os

import numpy as np
import pytest

from test_verdict_proof import _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sixteenth_header_and_ticket_signatures_agree():
    from neural_astar import _native
    protos = _prototypes("nastar_ticket.h")
    assert sorted(protos) == sorted(_native.TICKET_SIGNATURES) == ["nastar_forward_proved", "nastar_proof_order_counts", "nastar_proof_ticket_available",
                                                                  "nastar_ticket_abi"]
    for name, (ret, args) in protos.items():
        assert ret == "i", name
        assert _native.TICKET_SIGNATURES[name] == ret + " " + "".join(k for k, _ in args), name
    for other in (_native.SIGNATURES, _native.LEVEL_SIGNATURES, _native.VERDICT_SIGNATURES):
        assert not set(_native.TICKET_SIGNATURES) & set(other)  # a table of its own
    # the arguments of nastar_forward_ex without its stream, then levels and the proof's, then the stream
    ex = [n for _, n in _prototypes("nastar.h")["nastar_forward_ex"][1]]
    assert [n for _, n in protos["nastar_forward_proved"][1]] == ex[:-1] + ["levels", "proved_out", "proof_word", "proof_counter", "proof_rc", "stream"]
    for hdr in ("nastar.h", "nastar_levels.h", "nastar_verdict.h"):
        assert "ticket" not in open(os.path.join(ROOT, "include", hdr)).read().lower(), hdr


def test_library_exports_and_binds_the_ticket_symbols():
    from neural_astar import _native
    lib = _native.load()
    for sym in _native.TICKET_SIGNATURES:
        assert hasattr(lib, sym), sym
    assert lib.nastar_ticket_abi() == 1
    assert len(lib.nastar_forward_proved.argtypes) == 28
    assert _native.forward_proved_address() != 0


def test_a_null_proof_rc_is_refused_before_any_launch():
    from neural_astar import _native
    lib = _native.load()
    p = 0x10000  # never dereferenced
    assert lib.nastar_forward_proved(p, p, p, p, 2, 32, 32, 0.5, 1024, p, p, None, p, p, None, None, 0, 0, None, None, None, None, None, None, p, p,
                                     None, None) == 5


@pytest.mark.parametrize("B,W", [(1, 32), (3, 32), (129, 32), (3, 64)])
def test_the_mixed_batches_hold_the_kinds_they_name(B, W):
    import proof_ticket_cases as C
    for shift in range(len(C.KINDS)):
        m, s, g, kinds = C.mixed_batch(B, W, shift)
        want = C.flood_proved(m, s, g)
        assert [bool(w) for w in want] == [k in ("solvable", "start_is_goal") for k in kinds]
        assert (np.count_nonzero(s.reshape(B, -1), axis=1) == [0 if k == "no_start" else 1 for k in kinds]).all()
        if B >= len(C.KINDS):
            assert set(kinds) == set(C.KINDS) and m.max() == C.OVER[W]
