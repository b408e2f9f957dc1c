"""CPU: the C-ABI shared library builds for gfx950, loads, and exports every symbol include/nastar.h declares.
No compute call is made (there is no GPU here)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    txt = open(os.path.join(ROOT, "include", "nastar.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(nastar_[a-z0-9_]+)\s*\(", txt)))


def test_header_and_binding_agree():
    from neural_astar import _native
    assert _declared_symbols() == sorted(_native.EXPORTED_SYMBOLS)


_SCALARS = {"int": "i", "unsigned": "u", "float": "f", "double": "d", "size_t": "z", "long long": "q"}
_RETURNS = {"int": "i", "size_t": "z", "const char*": "s"}


def _prototypes():
    """include/nastar.h -> {symbol: (return kind, [(argument kind, argument name), ...])} in the letters of _native.SIGNATURES: p pointer,
    P pointer to pointer, i int, u unsigned, f float, d double, z size_t, q long long; returns i / z / s (const char*).  A type this does
    not know raises."""
    txt = open(os.path.join(ROOT, "include", "nastar.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    txt = re.sub(r"^\s*#.*$", "", txt, flags=re.M)
    out = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w \*]*?)\s*\b(nastar_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", txt):
        args = []
        for prm in (x.strip() for x in params.split(",")):
            if prm == "void":
                continue
            typ, arg = re.fullmatch(r"(.*?)(\w+)", prm).groups()
            stars = typ.count("*")
            base = " ".join(w for w in typ.replace("*", " ").split() if w not in ("const", "volatile"))
            if stars:
                assert stars <= 2 and re.fullmatch(r"void|float|double|long long|u?int\d+_t|int", base), (name, prm)
                args.append(("pP"[stars - 1], arg))
            else:
                assert base in _SCALARS, (name, prm)
                args.append((_SCALARS[base], arg))
        ret = " ".join(ret.replace("*", " * ").split()).replace(" *", "*")
        assert ret in _RETURNS, (name, ret)
        out[name] = (_RETURNS[ret], args)
    return out


def _defines():
    txt = open(os.path.join(ROOT, "include", "nastar.h")).read()
    return {k: int(v, 0) for k, v in re.findall(r"^#define (NASTAR_[A-Z0-9_]+) (0x[0-9A-Fa-f]+|\d+)\b", txt, flags=re.M)}


def test_signature_table_and_constants_match_the_header():
    """every prototype of include/nastar.h against _native.SIGNATURES (the ONE place the ctypes signatures come from): return type,
    parameter count, kind per position -- and the Python mirrors of the header's #defines against their values"""
    from neural_astar import _native, ops
    protos = _prototypes()
    assert sorted(protos) == sorted(_native.SIGNATURES) == _declared_symbols() and len(protos) == 74
    for name, (ret, args) in protos.items():
        assert _native.SIGNATURES[name] == ret + " " + "".join(k for k, _ in args), name
    assert set("".join(_native.SIGNATURES.values())) - {" "} <= set(_native._CTYPES)
    d = _defines()
    mirrors = {k: v for k, v in vars(ops).items() if k.startswith(("FLAG_", "STATUS_", "SUMMARY_", "NEIGHBORS_")) and isinstance(v, int)}
    assert {"FLAG_UNIT_COST", "FLAG_LOCKSTEP", "FLAG_CHECK_ORDER", "FLAG_MARK_COUPLED", "STATUS_UNSOLVABLE", "STATUS_NOT_UNIT_COST",
            "STATUS_BAD_HEURISTIC", "SUMMARY_WORDS", "SUMMARY_BAD_ORDER", "SUMMARY_COUPLED", "NEIGHBORS_MOORE8", "NEIGHBORS_VON_NEUMANN"} <= set(mirrors)
    for k, v in mirrors.items():
        assert v == d["NASTAR_" + k.replace("STATUS_", "ERR_")], k
    codes = {k: v for k, v in d.items() if k == "NASTAR_OK" or k.startswith("NASTAR_ERR_")}
    assert codes == {k: v for k, v in vars(_native).items() if k in codes} and len(codes) == 9
    assert sorted(_native._ERR_NAMES) == sorted(v for v in codes.values() if v)
    assert ops.SUMMARY_ERRORS == slice(1, ops.SUMMARY_COUPLED)


class _Sentinels:
    """distinct integers, one per name asked for"""

    def __init__(self):
        self.v = {}

    def __call__(self, name):
        return self.v.setdefault(name, 0x1000 + 0x10 * len(self.v))


def _check_call(call, expect, protos):
    """``call`` = (symbol, arguments) from an assembler; ``expect`` = header parameter name -> value: every parameter of the symbol's prototype is
    named in ``expect`` and holds that value; the stream is last"""
    name, args = call
    params = [n for _, n in protos[name][1]]
    assert len(args) == len(params), (name, len(args), len(params))
    assert params[-1] == "stream" and sorted(params) == sorted(expect), (name, sorted(set(params) ^ set(expect)))
    for prm, val in zip(params, args):
        assert val == expect[prm] and type(val) is type(expect[prm]), (name, prm, val, expect[prm])


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("family", ["", "_masked", "_heuristic", "_heuristic_moore8"])
def test_assembled_forward_calls_put_every_value_under_its_header_name(family, exact):
    """ops.forward_calls (what ops._launch_search issues) against the parameter NAMES of include/nastar.h, for the three entry families x
    exact on / off x every subset of the optional pointers"""
    import inspect
    import itertools
    from neural_astar import ops
    protos = _prototypes()
    header = [n for _, n in protos["nastar_forward_ex"][1]]
    # the assembler's own parameters ARE the header's, names and order (ops._launch_search passes them by position)
    assert list(inspect.signature(ops.forward_calls).parameters) == [n for n in header if n != "packed_out"] + ["exact", "neighbor_mask", "h0"]
    for opts in itertools.product([False, True], repeat=5):
        with_order, with_order_out, with_summary, with_counter, with_log = opts
        s = _Sentinels()
        mask = {"": None, "_masked": ops.NEIGHBORS_MOORE8, "_heuristic": ops.NEIGHBORS_VON_NEUMANN, "_heuristic_moore8": None}[family]
        h0 = s("h0") if family.startswith("_heuristic") else None
        suffix = family.replace("_moore8", "")
        given = {"cost": s("cost"), "start": s("start"), "goal": s("goal"), "passable": s("passable"), "B": 7, "H": 32, "W": 48, "g_ratio": 0.25,
                 "max_iters": 99, "histories_out": s("histories_out"), "paths_out": s("paths_out"), "sel_log_out": s("sel_log_out") if with_log else None,
                 "iters_out": s("iters_out"), "status_out": s("status_out"), "workspace": s("workspace") if exact else None,
                 "workspace_bytes": 4096 if exact else 0, "flags": ops.FLAG_MARK_COUPLED if exact else 0, "order": s("order") if with_order else None,
                 "order_out": s("order_out") if with_order_out else None, "status_summary": s("status_summary") if with_summary else 0,
                 "completion_counter": s("completion_counter") if with_counter else 0, "stream": s("stream")}
        launch, finish = ops.forward_calls(**given, exact=exact, neighbor_mask=mask, h0=h0)
        assert ops.forward_calls(*given.values(), exact, mask, h0) == (launch, finish)
        tail = {}
        if suffix:
            tail["neighbor_mask"] = ops.NEIGHBORS_MOORE8 if mask is None else mask
        if h0 is not None:
            tail["h0"] = h0
        assert launch[0] == "nastar_forward_ex" + suffix
        _check_call(launch, dict(given, packed_out=None, status_summary=given["status_summary"] or None,
                                 completion_counter=(given["completion_counter"] or None) if with_summary else None, **tail), protos)
        if exact:
            assert finish[0] == "nastar_forward_batchloop_finish" + suffix
            _check_call(finish, dict({k: given[k] for k in header[:14] + ["workspace", "workspace_bytes", "stream"]}, **tail), protos)
        else:
            assert finish is None


@pytest.mark.parametrize("case,symbol", [("plain", "nastar_backward_replay"), ("plain_flags", "nastar_backward_replay"),
                                         ("ordered", "nastar_backward_replay_ordered"), ("masked", "nastar_backward_replay_ordered_masked"),
                                         ("heuristic", "nastar_backward_replay_ordered_heuristic"),
                                         ("heuristic_masked_ordered", "nastar_backward_replay_ordered_heuristic"),
                                         ("l1", "nastar_backward_l1_replay"), ("l1_ordered", "nastar_backward_replay_ordered"),
                                         ("l1_flags", "nastar_backward_replay_ordered")])
def test_assembled_replay_calls_put_every_value_under_its_header_name(case, symbol):
    """ops.replay_call (what the two replay ops issue) against the parameter names of include/nastar.h, and WHICH symbol serves which call"""
    from neural_astar import ops
    protos = _prototypes()
    s = _Sentinels()
    l1 = case.startswith("l1")
    flags = ops.FLAG_LOCKSTEP if "flags" in case else 0
    order = s("order") if "ordered" in case else None
    mask = ops.NEIGHBORS_VON_NEUMANN if "masked" in case else None
    h0 = s("h0") if "heuristic" in case else None
    t_batch = None if case == "plain" else s("t_batch_dev")
    up = ({"histories": s("histories"), "opt_trajs": s("opt_trajs"), "grad_loss": s("grad_loss_dev") if case != "l1" else None} if l1
          else {"grad_hist": s("grad_histories")})
    call = ops.replay_call(cost=s("cost"), start=s("start"), goal=s("goal"), passable=s("passable"), sel_log=s("sel_log"), B=5, H=16, W=24, g_ratio=0.75,
                           max_iters=77, iters=s("iters"), t_batch=t_batch, grad_cost=s("grad_cost_out"), workspace=s("workspace"), ws_bytes=8192,
                           stream=s("stream"), flags=flags, order=order, neighbor_mask=mask, heuristic=h0, **up)
    assert call[0] == symbol
    expect = {"cost": s("cost"), "start": s("start"), "goal": s("goal"), "passable": s("passable"), "sel_log": s("sel_log"), "B": 5, "H": 16, "W": 24,
              "g_ratio": 0.75, "max_iters": 77, "iters": s("iters"), "t_batch_dev": t_batch, "grad_cost_out": s("grad_cost_out"),
              "workspace": s("workspace"), "workspace_bytes": 8192, "stream": s("stream")}
    if symbol != "nastar_backward_l1_replay":
        expect["flags"] = flags
    if symbol != "nastar_backward_replay":
        expect.update(histories=up.get("histories"), opt_trajs=up.get("opt_trajs"), grad_loss_dev=up.get("grad_loss"))
    if symbol != "nastar_backward_l1_replay":
        expect["grad_histories"] = up.get("grad_hist")
    if "_ordered" in symbol:
        expect["order"] = order
    if symbol.endswith(("_masked", "_heuristic")):
        expect["neighbor_mask"] = ops.NEIGHBORS_MOORE8 if mask is None else mask
    if symbol.endswith("_heuristic"):
        expect["h0"] = h0
    _check_call(call, expect, protos)


def test_library_builds_loads_and_exports_everything():
    from neural_astar import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    lib = _native.load()
    for sym in _declared_symbols():
        assert hasattr(lib, sym), sym
    hdr = open(os.path.join(ROOT, "include", "nastar.h")).read()
    assert lib.nastar_version() == int(re.search(r"#define NASTAR_VERSION (\d+)", hdr).group(1)) >= 300  # the library matches the header
    import neural_astar
    major, minor, patch = (int(x) for x in neural_astar.__version__.split("."))
    assert major * 1000 + minor * 100 + patch == lib.nastar_version()  # ... and the package names the same version
    assert lib.nastar_workspace_bytes(4096, 32, 32, 0) == 0
    assert lib.nastar_workspace_bytes(2, 79, 79, 0) == 0  # 9 B/cell compact state in LDS up to 6399 cells ...
    assert lib.nastar_workspace_bytes(2, 80, 80, 0) >= 2 * 80 * 80 * 5  # ... beyond, the large-map kernel (faster from 80x80 on: profiles/r06/probe_mid.jsonl)
    assert lib.nastar_workspace_bytes(2, 128, 128, 0) >= 2 * 128 * 128 * 5
    assert 2 * 200 * 150 * 5 <= lib.nastar_workspace_bytes(2, 200, 150, 0) < 2 * 200 * 150 * 6  # larger maps: 5 B/cell in the workspace (open list in LDS)
    # round 6: the marks of NASTAR_FLAG_MARK_COUPLED (B int32, 16-byte aligned, + the t_end cell) behind the slabs; the probe bitmaps of the finish call behind those
    assert lib.nastar_workspace_bytes(6, 32, 32, 32768) == 32 + 16 and lib.nastar_workspace_bytes(6, 32, 32, 32768 | 256) == 32 + 16 + 16
    assert lib.nastar_batchloop_workspace_bytes(6, 32, 32, 1024) == 32 + 16 + 16 + 6 * 32 * 4
    assert lib.nastar_batchloop_workspace_bytes(2, 200, 150, 22500) == lib.nastar_workspace_bytes(2, 200, 150, 32768 | 256) + 2 * 704 * 4
    assert lib.nastar_completion_supported(32, 32) == 1 and lib.nastar_completion_supported(200, 150) == 0
    assert lib.nastar_host_wait_nonzero(None, 10) == 0
    assert lib.nastar_backward_workspace_bytes(4, 32, 32, 256) >= 4 * 258 * 16  # replay backward: 16 B of history per step
    assert lib.nastar_last_error() == b""


def test_argument_validation_needs_no_gpu():
    """Status codes for bad arguments are produced before any HIP call."""
    from neural_astar import _native
    lib = _native.load()
    one = 16  # any non-NULL pointer value; never dereferenced on these paths
    assert lib.nastar_forward(None, one, one, one, 1, 8, 8, 0.5, 64, one, one, None, one, one, None, 0, 0, None) == _native.NASTAR_ERR_NULL
    assert lib.nastar_forward(one, one, one, one, 0, 8, 8, 0.5, 64, one, one, None, one, one, None, 0, 0, None) == _native.NASTAR_ERR_BAD_SHAPE
    assert lib.nastar_forward(one, one, one, one, 1, 8, 8, 0.5, 0, one, one, None, one, one, None, 0, 0, None) == _native.NASTAR_ERR_BAD_SHAPE
    assert lib.nastar_forward(one, one, one, one, 1, 2048, 2048, 0.5, 64, one, one, None, one, one, None, 0, 0, None) == _native.NASTAR_ERR_UNSUPPORTED
    assert lib.nastar_forward(one, one, one, one, 1, 1024, 1024, 0.5, 64, one, one, None, one, one, None, 0, 0, None) == _native.NASTAR_ERR_NULL  # (round 6: a supported size, it wants its workspace)
    assert lib.nastar_workspace_bytes(1, 1024, 1024, 0) >= 5 * 1024 * 1024 and lib.nastar_workspace_bytes(1, 1024, 1153, 0) == 0
    assert lib.nastar_forward(one, one, one, one, 1, 200, 150, 0.5, 64, one, one, None, one, one, one, 16, 0, None) == _native.NASTAR_ERR_WORKSPACE
    assert lib.nastar_forward(one, one, one, one, 1, 200, 150, 0.5, 64, one, one, None, one, one, None, 0, 0, None) == _native.NASTAR_ERR_NULL
    # placement: argument checks of nastar_forward carry over; maps whose state lives in HBM take none
    assert lib.nastar_forward_ordered(None, one, one, one, 1, 8, 8, 0.5, 64, one, one, None, one, one, None, None, 0, 0, one, one, None) == _native.NASTAR_ERR_NULL
    assert lib.nastar_forward_ordered(one, one, one, one, 0, 8, 8, 0.5, 64, one, one, None, one, one, None, None, 0, 0, one, None, None) == _native.NASTAR_ERR_BAD_SHAPE
    assert lib.nastar_forward_ordered(one, one, one, one, 1, 200, 150, 0.5, 64, one, one, None, one, one, None, one, 1 << 30, 0, one, None, None) == _native.NASTAR_ERR_UNSUPPORTED
    assert lib.nastar_forward_ordered(one, one, one, one, 1, 200, 150, 0.5, 64, one, one, None, one, one, None, one, 1 << 30, 0, None, one, None) == _native.NASTAR_ERR_UNSUPPORTED
    # nastar_forward_ex (0.5.0): the same checks; a CHECKED order needs its 16-byte verdict word in the workspace
    assert lib.nastar_forward_ex(None, one, one, one, 1, 8, 8, 0.5, 64, one, one, None, one, one, None, None, 0, 0, None, None, None, None, None) == _native.NASTAR_ERR_NULL
    assert lib.nastar_forward_ex(one, one, one, one, 1, 200, 150, 0.5, 64, one, one, None, one, one, None, one, 1 << 30, 0, one, None, None, None, None) == _native.NASTAR_ERR_UNSUPPORTED
    assert lib.nastar_workspace_bytes(4096, 32, 32, 256) == 16 and lib.nastar_workspace_bytes(4096, 32, 32, 0) == 0
    assert lib.nastar_forward_ex(one, one, one, one, 4, 32, 32, 0.5, 64, one, one, None, one, one, None, None, 0, 256, one, None, None, None, None) == _native.NASTAR_ERR_NULL
    assert lib.nastar_forward_ex(one, one, one, one, 4, 32, 32, 0.5, 64, one, one, None, one, one, None, one, 8, 256, one, None, None, None, None) == _native.NASTAR_ERR_WORKSPACE
    assert lib.nastar_placement_from_levels(None, 4, one, None) == _native.NASTAR_ERR_NULL
    assert lib.nastar_placement_from_levels(one, 0, one, None) == _native.NASTAR_ERR_BAD_SHAPE
    assert lib.nastar_backward_replay(None, one, one, one, one, one, 1, 8, 8, 0.5, 64, one, None, one, one, 64, 0, None) == _native.NASTAR_ERR_NULL
    # round 6: the A/B switches of earlier rounds (8 = NO_ASM, 16 / 128 = older streams, 32 = NO_DIVE, 512 = the round-4 large-map kernel, 2048.. = hybrid variants)
    # left the product ABI: unknown flag bits are refused (csrc/nastar_dev_flags.h, `make dev`)
    for bit in (8, 16, 32, 128, 512, 2048, 4096, 8192, 16384):
        assert lib.nastar_forward(one, one, one, one, 1, 8, 8, 0.5, 64, one, one, None, one, one, None, 0, bit, None) == _native.NASTAR_ERR_UNSUPPORTED, bit
    assert lib.nastar_forward_batchloop_finish(one, one, one, one, 2, 8, 8, 0.5, 64, one, one, None, one, one, None, 0, None) == _native.NASTAR_ERR_NULL
    assert lib.nastar_forward_batchloop_finish(one, one, one, one, 2, 8, 8, 0.5, 64, one, one, None, one, one, one, 16, None) == _native.NASTAR_ERR_WORKSPACE
    # the masked entry points (0.7.0): an invalid neighbor_mask (bits outside the 3x3 cells, or the centre) is refused before any other check
    vn = 0x0AA  # NASTAR_NEIGHBORS_VON_NEUMANN
    for bad in (0x10, 0x1FF, 0x200):
        assert lib.nastar_forward_ex_masked(None, one, one, one, 1, 8, 8, 0.5, 64, one, one, None, one, one, None, None, 0, 0, None, None, None, None, bad, None) == _native.NASTAR_ERR_UNSUPPORTED, bad
        assert lib.nastar_forward_batchloop_finish_masked(None, one, one, one, 2, 8, 8, 0.5, 64, one, one, None, one, one, None, 0, bad, None) == _native.NASTAR_ERR_UNSUPPORTED, bad
        assert lib.nastar_backward_replay_ordered_masked(None, None, None, None, one, one, one, one, one, 1, 8, 8, 0.5, 64, one, None, one, one, 1 << 20, 0, None, bad, None) == _native.NASTAR_ERR_UNSUPPORTED, bad
    assert lib.nastar_forward_ex_masked(None, one, one, one, 1, 8, 8, 0.5, 64, one, one, None, one, one, None, None, 0, 0, None, None, None, None, vn, None) == _native.NASTAR_ERR_NULL
    assert lib.nastar_forward_ex_masked(one, one, one, one, 0, 8, 8, 0.5, 64, one, one, None, one, one, None, None, 0, 0, None, None, None, None, vn, None) == _native.NASTAR_ERR_BAD_SHAPE
    assert lib.nastar_forward_ex_masked(one, one, one, one, 1, 200, 150, 0.5, 64, one, one, None, one, one, None, one, 1 << 30, 0, one, None, None, None, vn, None) == _native.NASTAR_ERR_UNSUPPORTED
    assert lib.nastar_forward_ex_masked(one, one, one, one, 4, 32, 32, 0.5, 64, one, one, None, one, one, None, one, 8, 256, one, None, None, None, vn, None) == _native.NASTAR_ERR_WORKSPACE
    assert lib.nastar_forward_batchloop_finish_masked(None, one, one, one, 2, 8, 8, 0.5, 64, one, one, None, one, one, one, 1 << 20, vn, None) == _native.NASTAR_ERR_NULL
    assert lib.nastar_forward_batchloop_finish_masked(one, one, one, one, 2, 8, 8, 0.5, 64, one, one, None, one, one, None, 0, vn, None) == _native.NASTAR_ERR_NULL
    assert lib.nastar_forward_batchloop_finish_masked(one, one, one, one, 2, 8, 8, 0.5, 64, one, one, None, one, one, one, 16, vn, None) == _native.NASTAR_ERR_WORKSPACE
    assert lib.nastar_backward_replay_ordered_masked(None, None, None, None, one, one, one, one, one, 1, 8, 8, 0.5, 64, one, None, one, one, 1 << 20, 0, None, vn, None) == _native.NASTAR_ERR_NULL
    assert lib.nastar_backward_replay_ordered_masked(one, None, None, None, None, one, one, one, one, 1, 8, 8, 0.5, 64, one, None, one, one, 1 << 20, 0, None, vn, None) == _native.NASTAR_ERR_NULL
    assert lib.nastar_backward_replay_ordered_masked(one, None, None, None, one, one, one, one, one, 0, 8, 8, 0.5, 64, one, None, one, one, 1 << 20, 0, None, vn, None) == _native.NASTAR_ERR_BAD_SHAPE
    assert lib.nastar_backward_replay_ordered_masked(one, None, None, None, one, one, one, one, one, 1, 8, 8, 0.5, 64, one, None, one, one, 16, 0, None, vn, None) == _native.NASTAR_ERR_WORKSPACE
    for sym in ("nastar_backward", "nastar_backward_l1", "nastar_has_dev_kernels"):  # rounds 1-3 legacy entry points: gone in 0.4.0
        assert not hasattr(lib, sym), sym
    assert lib.nastar_heuristic(None, 1, 8, 8, one, None) == _native.NASTAR_ERR_NULL
    # training / data-path / encoder entry points
    assert lib.nastar_l1_loss(one, None, 64, one, one, 2048, None) == _native.NASTAR_ERR_NULL
    assert lib.nastar_l1_loss(one, one, 0, one, one, 2048, None) == _native.NASTAR_ERR_BAD_SHAPE
    assert lib.nastar_l1_loss(one, one, 64, one, one, 8, None) == _native.NASTAR_ERR_WORKSPACE
    assert lib.nastar_policy_rollout(one, None, one, 1, 1, 8, 8, 8, one, one, None) == _native.NASTAR_ERR_NULL
    assert lib.nastar_policy_rollout(one, one, one, 1, 1, 9, 8, 8, one, one, None) == _native.NASTAR_ERR_BAD_SHAPE
    import ctypes
    arr = (ctypes.c_void_p * 5)(*([one] * 5))
    assert lib.nastar_encoder_cnn_forward(None, one, one, 1, 1, 32, 32, arr, arr, arr, 1.0, one, one, 1 << 20, None) == _native.NASTAR_ERR_NULL
    assert lib.nastar_encoder_cnn_forward(one, one, one, 1, 1, 30, 32, arr, arr, arr, 1.0, one, one, 1 << 20, None) == _native.NASTAR_ERR_UNSUPPORTED
    assert lib.nastar_encoder_cnn_forward(one, one, one, 1, 1, 32, 32, arr, arr, arr, 1.0, one, one, 16, None) == _native.NASTAR_ERR_WORKSPACE
    assert lib.nastar_encoder_workspace_bytes(4096, 32, 32) == 4096 * 1024 * 800 and lib.nastar_encoder_workspace_bytes(0, 32, 32) == 0
    assert lib.nastar_conv3x3_bf16(one, one, one, one, None, 1, 32, 32, 32, 64, 1, None) == _native.NASTAR_ERR_NULL
    assert lib.nastar_pack_outputs(None, one, 1, 8, 8, one, None) == _native.NASTAR_ERR_NULL
    assert lib.nastar_unpack_outputs(one, 0, 8, 8, one, one, None) == _native.NASTAR_ERR_BAD_SHAPE


def _validation_table():
    """[(symbol, a call that would pass every check, [(the arguments changed, the status that change must give), ...])] for the entry points
    of csrc/nastar_encoder_train_capi.hip, csrc/nastar_encoder_capi.hip and nastar_cost_to_go*: one change per status an entry point can
    return before its first HIP call.  The unchanged call is never made: with these pointers it would reach a launch."""
    import ctypes
    from neural_astar import _native as n
    NULL, SHAPE, UNSUP, WS = n.NASTAR_ERR_NULL, n.NASTAR_ERR_BAD_SHAPE, n.NASTAR_ERR_UNSUPPORTED, n.NASTAR_ERR_WORKSPACE
    o, o2, odd = 16, 32, 24  # non-NULL pointer values, never dereferenced on these paths; `odd` is not 16-byte aligned
    arr = (ctypes.c_void_p * 5)(*([o] * 5))
    big = 1 << 40
    t = []

    def entry(symbol, base, *cases):
        t.append((symbol, base, cases))

    def chan(C="C"):  # the channel layout of the streaming kernels: a multiple of 8, at most 2048, C / 8 divides 256
        return [({C: 12}, UNSUP), ({C: 24}, UNSUP), ({C: 4096}, UNSUP)]

    # ---- csrc/nastar_encoder_train_capi.hip
    entry("nastar_conv3x3_wgrad_f16",
          dict(dz=o, a=o, dw=o, B=1, H=32, W=32, co=32, ci=32, co_real=32, ci_real=32, split=0, out_scale=1.0, grad_scale_dev=None, workspace=o,
               workspace_bytes=big, stream=None),
          ({"dz": None}, NULL), ({"workspace": None}, NULL), ({"B": 0}, SHAPE), ({"co_real": 33}, SHAPE), ({"ci_real": 0}, SHAPE),
          ({"co": 48, "co_real": 48}, UNSUP), ({"ci": 16, "ci_real": 16}, UNSUP), ({"dz": odd}, SHAPE), ({"workspace": odd}, SHAPE),
          ({"workspace_bytes": 0}, WS), ({"split": 1, "workspace_bytes": 9 * 32 * 32 * 4 - 1}, WS))
    entry("nastar_chan_stats_f16", dict(u=o, v=o, ms=o, mt=o, sums=o, amax_out=o, npix=64, C=8, split=0, stream=None),
          ({"v": None}, NULL), ({"sums": None}, NULL), ({"ms": None}, NULL), ({"npix": 0}, SHAPE), ({"C": 0}, SHAPE), *chan())
    entry("nastar_chan_stats_f16_ws",
          dict(u=o, v=o, ms=o, mt=o, sums=o, amax_out=o, npix=64, C=8, split=0, workspace=o, workspace_bytes=big, stream=None),
          ({"v": None}, NULL), ({"workspace": None}, NULL), ({"mt": None}, NULL), ({"npix": 0}, SHAPE), *chan(), ({"workspace_bytes": 16}, WS))
    entry("nastar_bn_stats_coef_fwd_f16",
          dict(z=o, npix=64, C=8, split=0, gamma=o, beta=o, eps=1e-5, momentum=0.1, running_mean=o, running_var=o, k2=o, k3=o, mean_out=o,
               invstd_out=o, sums_out=None, workspace=o, workspace_bytes=big, stream=None),
          ({"z": None}, NULL), ({"k3": None}, NULL), ({"running_var": None}, NULL), ({"C": 0}, SHAPE), *chan(), ({"workspace_bytes": 16}, WS))
    entry("nastar_bn_stats_coef_bwd_f16",
          dict(da=o, z=o, ms=o, mt=o, npix=64, C=8, split=0, mean=o, invstd=o, gamma=o, gscale_in=o, gscale_out=o2, dgamma=o, dbeta=o, c1=o, c2=o,
               c3=o, sums_out=None, workspace=o, workspace_bytes=big, stream=None),
          ({"da": None}, NULL), ({"c3": None}, NULL), ({"npix": 0}, SHAPE), ({"gscale_out": o}, SHAPE), *chan(), ({"workspace_bytes": 16}, WS))
    entry("nastar_chan_affine_f16", dict(u=o, v=o, k1=o, k2=o, k3=o, ms=o, mt=o, out=o, npix=64, C=8, relu=1, split=0, stream=None),
          ({"v": None}, NULL), ({"k1": None}, NULL), ({"npix": 0}, SHAPE), *chan())
    entry("nastar_pack_conv_weight_f16",
          dict(w=o, co=32, ci=32, transpose_flip=0, split=0, bias=None, wpack=o, scale_out=o, shift_out=o, scal_out=o, reuse_max=0, stream=None),
          ({"w": None}, NULL), ({"scal_out": None}, NULL), ({"co": 0}, SHAPE), ({"ci": -1}, SHAPE))
    entry("nastar_absmax_multi_f32", dict(table=o, n=1, scal=o, stream=None), ({"table": None}, NULL), ({"n": 0}, SHAPE), ({"n": 65536}, SHAPE))
    entry("nastar_pack_conv_weights_multi_f16", dict(table=o, n=1, max_tiles=1, split=0, scal=o, flat16=o, flatf=o, stream=None),
          ({"flatf": None}, NULL), ({"n": 0}, SHAPE), ({"max_tiles": 0}, SHAPE), ({"max_tiles": 65536}, SHAPE))
    entry("nastar_rmsprop_multi_f32", dict(table=o, n=1, lr=1e-3, alpha=0.99, eps=1e-8, stream=None),
          ({"table": None}, NULL), ({"n": 0}, SHAPE), ({"n": 65536}, SHAPE))
    entry("nastar_bn_coef_fwd",
          dict(sums=o, gamma=o, beta=o, eps=1e-5, npix=64, momentum=0.1, running_mean=o, running_var=o, k2=o, k3=o, mean_out=o, invstd_out=o, C=8,
               stream=None),
          ({"sums": None}, NULL), ({"running_var": None}, NULL), ({"C": 0}, SHAPE), ({"npix": 0}, SHAPE))
    entry("nastar_bn_coef_bwd_io",
          dict(sums=o, amax_dy=o, mean=o, invstd=o, gamma=o, npix=64, gscale_in=o, gscale_out=o2, dgamma=o, dbeta=o, c1=o, c2=o, c3=o, C=8,
               stream=None),
          ({"amax_dy": None}, NULL), ({"gscale_in": None}, NULL), ({"C": 0}, SHAPE), ({"npix": 0}, SHAPE))
    entry("nastar_bn_coef_bwd",
          dict(sums=o, amax_dy=o, mean=o, invstd=o, gamma=o, npix=64, gscale=o, dgamma=o, dbeta=o, c1=o, c2=o, c3=o, C=8, stream=None),
          ({"gscale": None}, NULL), ({"C": 0}, SHAPE), ({"npix": 0}, SHAPE))
    entry("nastar_grad_seed_f16", dict(d=o, npix=64, split=0, dzb=o, gscale=o, amax_scratch=o, stream=None),
          ({"d": None}, NULL), ({"amax_scratch": None}, NULL), ({"npix": 0}, SHAPE))
    entry("nastar_maxpool2x2_bwd_f16", dict(r=o, dp=o, dr=o, B=1, H=8, W=8, C=8, split=0, stream=None),
          ({"dr": None}, NULL), ({"B": 0}, SHAPE), ({"H": 7}, UNSUP), ({"C": 12}, UNSUP))
    for sym, ptrs in (("nastar_upcat_f16", ("x", "skip", "out")), ("nastar_upcat_bwd_f16", ("dcat", "dx", "dskip"))):
        opt = ptrs[1] if sym == "nastar_upcat_f16" else ptrs[2]  # the pointer that may be NULL when c2 == 0
        entry(sym, dict(**{p: o for p in ptrs}, B=1, H=8, W=8, c1=8, c2=8, split=0, stream=None),
              ({ptrs[0]: None}, NULL), ({opt: None}, NULL), ({"B": 0}, SHAPE), ({"c2": -8}, SHAPE), ({"W": 7}, UNSUP), ({"c1": 12}, UNSUP))
    entry("nastar_grad_add_f16", dict(a=o, scale_a=o, b=o, scale_b=o, out=o, scale_out=o, npix=64, C=8, split=0, stream=None),
          ({"b": None}, NULL), ({"scale_out": None}, NULL), ({"npix": 0}, SHAPE), ({"C": 12}, UNSUP))
    entry("nastar_bn1_fwd_partial", dict(z=o, n=64, part=o, stream=None), ({"z": None}, NULL), ({"part": None}, NULL), ({"n": 0}, SHAPE))
    entry("nastar_bn1_sigmoid_fwd",
          dict(z=o, n=64, part=o, nparts=1, n_total=64.0, gamma=o, beta=o, eps=1e-5, cmul=None, momentum=0.1, running_mean=o, running_var=o,
               cost_out=o, stat_out=o, stream=None),
          ({"z": None}, NULL), ({"running_var": None}, NULL), ({"n": 0}, SHAPE), ({"nparts": 0}, SHAPE), ({"nparts": 257}, SHAPE),
          ({"n_total": 63.0}, SHAPE))
    entry("nastar_bn1_sigmoid_bwd_partial", dict(z=o, dcost=o, n=64, stat=o, gamma=o, beta=o, cmul=None, part=o, stream=None),
          ({"dcost": None}, NULL), ({"part": None}, NULL), ({"n": 0}, SHAPE))
    entry("nastar_bn1_sigmoid_bwd",
          dict(z=o, dcost=o, n=64, stat=o, gamma=o, beta=o, cmul=None, part=o, nparts=1, n_total=64.0, dz_out=o, dgamma_out=o, dbeta_out=o,
               dconst_out=None, stream=None),
          ({"stat": None}, NULL), ({"dbeta_out": None}, NULL), ({"n": 0}, SHAPE), ({"nparts": 257}, SHAPE), ({"n_total": 63.0}, SHAPE))
    co1 = [({"B": 0}, SHAPE), ({"C": 0}, SHAPE), ({"C": 4}, UNSUP), ({"C": 24}, UNSUP), ({"C": 1024}, UNSUP), ({"workspace_bytes": 16}, WS)]
    entry("nastar_conv3x3_co1_f16",
          dict(a=o, w=o, bias=None, B=1, H=8, W=8, C=8, split=0, k2=o, k3=o, z_out=o, workspace=o, workspace_bytes=big, stream=None),
          ({"a": None}, NULL), ({"workspace": None}, NULL), ({"k3": None}, NULL), *co1)
    entry("nastar_conv3x3_co1_wgrad_f16",
          dict(d=o, a=o, B=1, H=8, W=8, C=8, split=0, k2=o, k3=o, dw_out=o, workspace=o, workspace_bytes=big, stream=None),
          ({"d": None}, NULL), ({"dw_out": None}, NULL), ({"k3": None}, NULL), *co1)
    entry("nastar_grad_scale_f32", dict(d=o, npix=64, gscale=o, amax_scratch=o, stream=None),
          ({"d": None}, NULL), ({"gscale": None}, NULL), ({"npix": 0}, SHAPE))
    entry("nastar_chan_stats_u1_f16_ws",
          dict(d=o, wlast=o, gscale=o, B=1, H=8, W=8, v=o, ms=o, mt=o, sums=o, amax_out=None, C=8, split=0, workspace=o, workspace_bytes=big,
               stream=None),
          ({"wlast": None}, NULL), ({"sums": None}, NULL), ({"H": 0}, SHAPE), ({"C": 0}, SHAPE), *chan(), ({"workspace_bytes": 16}, WS))
    entry("nastar_bn_stats_coef_bwd_u1_f16",
          dict(d=o, wlast=o, B=1, H=8, W=8, z=o, ms=o, mt=o, C=8, split=0, mean=o, invstd=o, gamma=o, gscale_in=o, gscale_out=o2, dgamma=o,
               dbeta=o, c1=o, c2=o, c3=o, sums_out=None, workspace=o, workspace_bytes=big, stream=None),
          ({"d": None}, NULL), ({"workspace": None}, NULL), ({"W": 0}, SHAPE), ({"gscale_out": o}, SHAPE), *chan(), ({"workspace_bytes": 16}, WS))
    entry("nastar_chan_affine_u1_f16",
          dict(d=o, wlast=o, gscale=o, B=1, H=8, W=8, z=o, k1=o, k2=o, k3=o, ms=o, mt=o, out=o, C=8, split=0, stream=None),
          ({"gscale": None}, NULL), ({"out": None}, NULL), ({"B": 0}, SHAPE), *chan())
    # ---- csrc/nastar_encoder_capi.hip
    entry("nastar_encoder_cnn_forward",
          dict(map=o, start=o, goal=o, plus=1, B=1, H=32, W=32, wpack=arr, scale=arr, shift=arr, final_mul=1.0, cost_out=o, workspace=o,
               workspace_bytes=big, stream=None),
          ({"cost_out": None}, NULL), ({"wpack": None}, NULL), ({"goal": None}, NULL), ({"B": 0}, SHAPE), ({"W": 40}, UNSUP),
          ({"workspace_bytes": 32 * 32 * 800 - 1}, WS))
    for sym, per_pixel in (("nastar_encoder_cnn_forward_f16x3", 2 * 480 * 2 + 4), ("nastar_encoder_cnn_forward_f16", 480 * 2 + 4)):
        entry(sym,
              dict(map=o, start=o, goal=o, plus=1, B=1, H=32, W=32, w1_f32=o, wts=arr, scale=arr, shift=arr, final_mul=1.0, cost_out=o,
                   workspace=o, workspace_bytes=big, stream=None),
              ({"map": None}, NULL), ({"w1_f32": None}, NULL), ({"start": None}, NULL), ({"shift": None}, NULL), ({"H": 0}, SHAPE),
              ({"H": 48}, UNSUP), ({"workspace_bytes": 32 * 32 * per_pixel - 1}, WS))
    entry("nastar_conv3x3_bf16", dict(inp=o, wpack=o, scale=o, shift=o, out=o, B=1, H=32, W=32, cin=32, cout=64, relu=1, stream=None),
          ({"inp": None}, NULL), ({"B": 0}, SHAPE), ({"H": 30}, SHAPE), ({"cin": 48}, UNSUP), ({"cout": 32}, UNSUP))
    entry("nastar_encoder_cnn_downsize_forward",
          dict(image=o, start=o, goal=o, plus=1, B=1, C=3, H=32, W=32, h=4, w=4, depth=3, wts=arr, scale=arr, shift=arr, final_mul=1.0,
               cost_out=o, workspace=o, workspace_bytes=big, stream=None),
          ({"image": None}, NULL), ({"goal": None}, NULL), ({"workspace": None}, NULL), ({"depth": 5}, SHAPE), ({"C": 4}, SHAPE),
          ({"H": 36}, UNSUP), ({"h": 0}, UNSUP), ({"workspace_bytes": 16}, WS))
    entry("nastar_conv3x3_img32_f16", dict(inp=o, wpack=o, scale=o, shift=o, out=o, B=1, cin=32, cout=64, flags=1, stream=None),
          ({"scale": None}, NULL), ({"B": 0}, SHAPE), ({"out": odd}, SHAPE), ({"flags": 2}, UNSUP), ({"cin": 48}, UNSUP), ({"cout": 256}, UNSUP))
    entry("nastar_conv3x3_f16",
          dict(inp=o, in2=o, wpack=o, scale=o, shift=o, out=o, out_f32=None, B=1, H=8, W=8, c1=32, c2=32, cout=32, flags=1, final_mul=1.0,
               stream=None),
          ({"inp": None}, NULL), ({"out": None}, NULL), ({"in2": None}, NULL), ({"flags": 2}, NULL), ({"B": 0}, SHAPE), ({"c2": -32}, SHAPE),
          ({"c1": 16}, UNSUP), ({"cout": 48}, UNSUP), ({"flags": 2, "out_f32": o, "cout": 64}, UNSUP), ({"flags": 4, "H": 7}, UNSUP),
          ({"B": 1 << 20, "H": 64, "W": 64}, UNSUP), ({"in2": odd}, SHAPE))
    entry("nastar_maxpool2x2_f16", dict(inp=o, out=o, B=1, H=8, W=8, C=8, split=0, stream=None),
          ({"out": None}, NULL), ({"C": 0}, SHAPE), ({"W": 7}, UNSUP), ({"C": 12}, UNSUP))
    entry("nastar_encoder_prep_f16", dict(map=o, start=o, goal=o, plus=1, npix=64, cp=8, split=0, out=o, stream=None),
          ({"out": None}, NULL), ({"start": None}, NULL), ({"npix": 0}, SHAPE), ({"cp": 1}, SHAPE), ({"cp": 12}, SHAPE))
    # ---- nastar_cost_to_go* (include/nastar_fields.h, include/nastar_fields_tiled.h): an invalid neighbor_mask is refused before any other check
    field = dict(cost=o, goal=o, passable=o, B=1, H=8, W=8, neighbor_mask=0x1EF, dist_out=o, policy_out=None, status_out=o)
    field_cases = [({"neighbor_mask": 0x10, "cost": None}, UNSUP), ({"neighbor_mask": 0x200}, UNSUP), ({"cost": None}, NULL),
                   ({"status_out": None}, NULL), ({"B": 0}, SHAPE)]
    entry("nastar_cost_to_go", dict(field, stream=None), *field_cases, ({"H": 128, "W": 129}, UNSUP))
    entry("nastar_cost_to_go_sweeps", dict(field, sweeps_out=None, stream=None), *field_cases, ({"H": 128, "W": 129}, UNSUP))
    tiled = dict(field, visits_out=None, workspace=o, workspace_bytes=big, max_rounds=0)
    tiled_cases = field_cases + [({"workspace": None}, NULL), ({"max_rounds": -1}, SHAPE), ({"H": 1024, "W": 1153}, UNSUP),
                                 ({"workspace_bytes": 16}, WS), ({"workspace": 18}, WS)]
    entry("nastar_cost_to_go_tiled", dict(tiled, rounds_out=None, stream=None), *tiled_cases)
    entry("nastar_cost_to_go_tiled_batched", dict(tiled, launches_per_batch=0, rounds_out=None, stream=None), *tiled_cases,
          ({"launches_per_batch": -1}, SHAPE))
    return t


def test_argument_validation_table_needs_no_gpu():
    """The training, encoder and cost-to-go entry points: every status an entry point can return before its first HIP call, one call each
    (_validation_table).  Every call differs from a valid one by the change under test, so none gets past the argument checks."""
    from neural_astar import _native
    lib = _native.load()
    signatures = dict(_native.SIGNATURES, **_native.FIELD_SIGNATURES, **_native.TILED_FIELD_SIGNATURES)
    table = _validation_table()
    seen = {}
    for symbol, base, cases in table:
        assert len(base) == len(signatures[symbol].split(" ")[1]) and list(base)[-1] == "stream", symbol
        for change, status in cases:
            assert change and set(change) <= set(base) and any(base[k] != v for k, v in change.items()), (symbol, change)
            assert status in (_native.NASTAR_ERR_NULL, _native.NASTAR_ERR_BAD_SHAPE, _native.NASTAR_ERR_UNSUPPORTED, _native.NASTAR_ERR_WORKSPACE)
            assert getattr(lib, symbol)(*dict(base, **change).values()) == status, (symbol, change)
            seen.setdefault(symbol, set()).add(status)
    # every status-returning entry point the two encoder translation units define is in the table (nastar_bn1_parts returns a count) ...
    csrc = os.path.join(ROOT, "neural-astar_amd", "csrc")
    defined = set()
    for f in ("nastar_encoder_train_capi.hip", "nastar_encoder_capi.hip"):
        defined |= set(re.findall(r"^int (nastar_[a-z0-9_]+)\(", open(os.path.join(csrc, f)).read(), flags=re.M))
    defined |= {s for s in signatures if s.startswith("nastar_cost_to_go") and not s.endswith("_bytes")}
    assert defined - {"nastar_bn1_parts"} == set(seen) and len(seen) == len(table) == 41
    # ... with a NULL and a BAD_SHAPE call each, and a WORKSPACE call wherever a workspace size is passed
    for symbol, base, _ in table:
        need = {_native.NASTAR_ERR_NULL, _native.NASTAR_ERR_BAD_SHAPE} | ({_native.NASTAR_ERR_WORKSPACE} if "workspace_bytes" in base else set())
        assert need <= seen[symbol], (symbol, seen[symbol])
    assert lib.nastar_bn1_parts(0) == 0 and lib.nastar_bn1_parts(1) == 1 and lib.nastar_bn1_parts(1 << 40) == 256
    assert lib.nastar_last_error() == b""  # no call reached the HIP runtime


def test_eval_encoder_refusals_need_no_gpu():
    """The three forward entry points of the eval-mode CNN encoder refuse, before any HIP call: a workspace smaller than one image (the
    size is the library's own nastar_encoder_workspace_bytes*(1, H, W)), map heights their kernels do not tile, `plus` without a start
    map, and an empty batch."""
    import ctypes
    from neural_astar import _native as n
    lib = n.load()
    o = 16  # a non-NULL pointer value, never dereferenced on these paths
    arr = (ctypes.c_void_p * 5)(*([o] * 5))
    big = 1 << 40
    forms = [("nastar_encoder_cnn_forward", "nastar_encoder_workspace_bytes", (), 20),
             ("nastar_encoder_cnn_forward_f16", "nastar_encoder_workspace_bytes_f16", (o,), 16),
             ("nastar_encoder_cnn_forward_f16x3", "nastar_encoder_workspace_bytes_f16x3", (o,), 16)]
    for fwd_name, ws_name, w1, bad_h in forms:
        fwd, ws_fn = getattr(lib, fwd_name), getattr(lib, ws_name)

        def call(start=o, plus=1, B=3, H=32, W=32, ws_bytes=big):
            return fwd(o, start, o, plus, B, H, W, *w1, arr, arr, arr, 1.0, o, o, ws_bytes, None)

        for H, W in ((32, 32), (64, 96)):
            per_image = int(ws_fn(1, H, W))
            assert per_image > 0 and int(ws_fn(3, H, W)) == 3 * per_image
            assert call(H=H, W=W, ws_bytes=per_image - 1) == n.NASTAR_ERR_WORKSPACE, (fwd_name, H, W)
            assert call(H=H, W=W, ws_bytes=0) == n.NASTAR_ERR_WORKSPACE, (fwd_name, H, W)
        assert call(H=bad_h) == n.NASTAR_ERR_UNSUPPORTED, fwd_name
        assert call(start=None) == n.NASTAR_ERR_NULL, fwd_name
        assert call(B=0) == n.NASTAR_ERR_BAD_SHAPE, fwd_name
    assert lib.nastar_last_error() == b""  # no call reached the HIP runtime


def test_product_has_no_cpu_fallback_and_never_touches_the_oracle():
    import torch
    from neural_astar.planner import VanillaAstar
    x = torch.ones(1, 1, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU"):
        VanillaAstar()(x, x, x)
    pkg = os.path.join(ROOT, "neural-astar_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(dp, f)).read()
                assert "import oracle" not in src and "from oracle" not in src and "nastar_oracle" not in src, f
