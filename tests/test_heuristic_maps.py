"""CPU: the ``heuristic_maps`` argument of the planners (signature, validation before any launch, the "no CPU" error, a replaced
``get_heuristic``) and the argument checks of the C entry points that take a caller-supplied heuristic."""
import inspect
import os
import re

import pytest
import torch

from neural_astar import _native, ops
from neural_astar.planner import NeuralAstar, VanillaAstar
from neural_astar.planner.differentiable_astar import DifferentiableAstar


def test_the_keyword_exists_and_defaults_to_none():
    for fn in (DifferentiableAstar.forward, VanillaAstar.forward, NeuralAstar.forward, VanillaAstar.perform_astar, NeuralAstar.perform_astar):
        p = inspect.signature(fn).parameters
        assert "heuristic_maps" in p and p["heuristic_maps"].default is None, fn.__qualname__
        assert list(p)[-1] == "heuristic_maps", fn.__qualname__  # trailing: every positional call of the reference keeps its meaning
    for op in (ops.astar_forward, ops.astar_forward_ordered, ops.astar_backward_replay):
        assert "heuristic" in str(op._schema) and "Tensor? heuristic=None" in str(op._schema)


def _maps(B=2, H=8, W=8):
    x = torch.ones(B, 1, H, W)
    return x, x.clone(), x.clone(), x.clone()


@pytest.mark.parametrize("bad, exc", [
    (torch.zeros(2, 8, 8), ValueError),            # rank
    (torch.zeros(2, 1, 8, 9), ValueError),         # shape
    (torch.zeros(1, 1, 8, 8), ValueError),         # batch
    (torch.zeros(2, 2, 8, 8), ValueError),         # channels
    (torch.zeros(2, 1, 8, 8, dtype=torch.float64), TypeError),
    (torch.zeros(2, 1, 8, 8, dtype=torch.float16), TypeError),
    (torch.zeros(2, 1, 8, 8, device="meta"), ValueError),  # another device than cost_maps
    (lambda goal_maps: goal_maps, TypeError),      # a callable is not the interface
])
def test_bad_heuristic_maps_raise_before_anything_is_launched(bad, exc, monkeypatch):
    monkeypatch.setattr(_native, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was reached")))
    with pytest.raises(exc, match="heuristic_maps"):
        DifferentiableAstar()(*_maps(), heuristic_maps=bad)
    with pytest.raises(exc, match="heuristic_maps"):
        VanillaAstar()(*_maps()[:3], heuristic_maps=bad)


def test_cpu_tensors_keep_raising_the_no_cpu_error():
    c, s, g, p = _maps()
    with pytest.raises(RuntimeError, match="no CPU"):
        DifferentiableAstar()(c, s, g, p, heuristic_maps=torch.zeros(2, 1, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU"):
        VanillaAstar()(c, s, g, heuristic_maps=torch.zeros(2, 1, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU"):
        VanillaAstar().perform_astar(c, s, g, p, False, torch.zeros(2, 1, 8, 8))


def test_a_replaced_get_heuristic_still_raises_and_names_the_supported_route():
    m = DifferentiableAstar()
    m.get_heuristic = lambda goal_maps: torch.zeros_like(goal_maps)
    with pytest.raises(NotImplementedError, match="get_heuristic was replaced") as e:
        m(*_maps())
    assert "heuristic_maps" in str(e.value)
    with pytest.raises(NotImplementedError, match="get_heuristic was replaced"):  # ... also when the supported route is used beside it
        m(*_maps(), heuristic_maps=torch.zeros(2, 1, 8, 8))


def test_entry_points_check_their_arguments_in_the_documented_order():
    lib = _native.load()
    one = 16  # any non-NULL address: every call below is refused before a pointer is dereferenced
    ws = 1 << 20
    assert lib.nastar_version() == 800
    M = ops.NEIGHBORS_MOORE8

    def fwd(cost=one, B=1, flags=0, mask=M, h0=one, H=8, W=8):
        return lib.nastar_forward_ex_heuristic(cost, one, one, one, B, H, W, 0.5, 64, one, one, None, one, one, None, None, 0, flags, None, None, None,
                                               None, mask, h0, None)

    def fin(cost=one, B=2, mask=M, h0=one, wsp=one, wsb=ws):
        return lib.nastar_forward_batchloop_finish_heuristic(cost, one, one, one, B, 8, 8, 0.5, 64, one, one, None, one, one, wsp, wsb, mask, h0, None)

    def bwd(gh=one, B=1, mask=M, h0=one, wsb=ws):
        return lib.nastar_backward_replay_ordered_heuristic(gh, None, None, None, one, one, one, one, one, B, 8, 8, 0.5, 64, one, None, one, one, wsb, 0,
                                                            None, mask, h0, None)

    for bad in (0x1FF, 0x010, 0x200, 0xFFFFFFFF):  # an invalid mask comes first, whatever else is wrong
        assert fwd(mask=bad, h0=None, cost=None) == _native.NASTAR_ERR_UNSUPPORTED
        assert fin(mask=bad, h0=None) == _native.NASTAR_ERR_UNSUPPORTED
        assert bwd(mask=bad, h0=None) == _native.NASTAR_ERR_UNSUPPORTED
    for good in (M, ops.NEIGHBORS_VON_NEUMANN, 0):
        assert fwd(mask=good, h0=None) == _native.NASTAR_ERR_NULL      # a NULL heuristic
        assert fin(mask=good, h0=None) == _native.NASTAR_ERR_NULL
        assert bwd(mask=good, h0=None) == _native.NASTAR_ERR_NULL
        assert fwd(mask=good, h0=None, B=0) == _native.NASTAR_ERR_NULL  # ... before the shape
        assert fwd(mask=good, cost=None) == _native.NASTAR_ERR_NULL
        assert fwd(mask=good, B=0) == _native.NASTAR_ERR_BAD_SHAPE
        assert fwd(mask=good, flags=8) == _native.NASTAR_ERR_UNSUPPORTED  # unknown flag bits stay refused
        assert fwd(mask=good, H=2000, W=2000) == _native.NASTAR_ERR_UNSUPPORTED
        assert fin(mask=good, wsp=None, wsb=0) == _native.NASTAR_ERR_NULL
        assert fin(mask=good, wsb=16) == _native.NASTAR_ERR_WORKSPACE
        assert bwd(mask=good, gh=None) == _native.NASTAR_ERR_NULL
        assert bwd(mask=good, B=0) == _native.NASTAR_ERR_BAD_SHAPE
        assert bwd(mask=good, wsb=16) == _native.NASTAR_ERR_WORKSPACE


def test_header_library_and_package_name_the_new_status_and_symbols():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nastar.h")).read()
    assert int(re.search(r"#define NASTAR_ERR_BAD_HEURISTIC (\d+)", hdr).group(1)) == ops.STATUS_BAD_HEURISTIC == _native.NASTAR_ERR_BAD_HEURISTIC == 8
    assert ops.STATUS_BAD_HEURISTIC in range(*ops.SUMMARY_ERRORS.indices(16))  # a per-map code inside the summary's error cells
    for sym in ("nastar_forward_ex_heuristic", "nastar_forward_batchloop_finish_heuristic", "nastar_backward_replay_ordered_heuristic"):
        assert sym in _native.EXPORTED_SYMBOLS and re.search(r"\bint " + sym + r"\(", hdr)
