"""CPU: the in-launch placement by levels (include/nastar_levels.h) -- everything that needs no GPU.

1. the numpy restatement of the rule (tests/placement_rule.py) is a bijection for every batch size and level set the GPU tests use, puts
   the longest map of every block into the first row of workgroups, and orders a level-sorted batch almost exactly;
2. the fourth header against ``_native.LEVEL_SIGNATURES``; the library exports its symbols; ``nastar.h`` does not change;
3. the refusals of ``nastar_forward_levels`` (made before any HIP call, so they need no device) and ``nastar_levels_in_launch`` beside them.
"""
import os
import re

import numpy as np
import pytest

import placement_rule as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the rule ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", PR.BATCH_SIZES + (100, 1000, 4095, 10000))
def test_restatement_is_a_bijection(B):
    for name, lv in PR.level_sets(B).items():
        assert PR.is_permutation(PR.slots(lv), B), (B, name)


@pytest.mark.parametrize("B", [130, 4096, 4097])
def test_first_row_holds_the_longest_map_of_every_block(B):
    nblk = (B + 63) // 64
    for name, lv in PR.level_sets(B).items():
        o = PR.slots(lv)
        c = np.clip(lv.astype(np.int64), 0, PR.MAX_LEVEL)
        for j in range(nblk):
            assert c[o[j]] == c[j::nblk].max(), (B, name, j)
        # inside a block the ranks descend by level, the lower map first among equals
        blk = o[0::nblk]
        key = [(-c[m], m) for m in blk]
        assert key == sorted(key), (B, name)


def test_equal_levels_keep_the_natural_order_and_sorted_batches_stay_sorted():
    B = 4096
    assert np.array_equal(PR.slots(np.full(B, 3, np.int32)), np.arange(B))
    # a batch that arrives sorted by level: strided blocks see every part of it, the slots follow the exact rank closely
    lv = np.sort(np.random.default_rng(1).integers(0, 400, B).astype(np.int32))[::-1].copy()
    o = PR.slots(lv)
    exact_rank = np.empty(B, np.int64)
    exact_rank[np.argsort(-lv.astype(np.int64), kind="stable")] = np.arange(B)
    slot_of = np.empty(B, np.int64)
    slot_of[o] = np.arange(B)
    assert np.corrcoef(exact_rank, slot_of)[0, 1] > 0.99


# ---- 2. header and binding -----------------------------------------------------------------------------------------------------------
_SCALARS = {"int": "i", "unsigned": "u", "float": "f", "double": "d", "size_t": "z", "long long": "q"}


def _prototypes(header):
    """include/<header> -> {symbol: (return letter, [(kind letter, parameter name), ...])} in the letters of _native.SIGNATURES"""
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    txt = re.sub(r"^\s*#.*$", "", txt, flags=re.M)
    out = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w \*]*?)\s*\b(nastar_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", txt):
        args = []
        for prm in (x.strip() for x in params.split(",")):
            if prm == "void":
                continue
            typ, arg = re.fullmatch(r"(.*?)(\w+)", prm).groups()
            base = " ".join(w for w in typ.replace("*", " ").split() if w != "const")
            args.append(("p" if "*" in typ else _SCALARS[base], arg))
        out[name] = ({"int": "i", "size_t": "z"}.get(ret.strip(), "s"), args)
    return out


def test_fourth_header_and_level_signatures_agree():
    from neural_astar import _native
    protos = _prototypes("nastar_levels.h")
    assert sorted(protos) == sorted(_native.LEVEL_SIGNATURES) == ["nastar_forward_levels", "nastar_levels_abi", "nastar_levels_in_launch",
                                                                  "nastar_placement_slots"]
    for name, (ret, args) in protos.items():
        assert ret == "i", name
        assert _native.LEVEL_SIGNATURES[name] == ret + " " + "".join(k for k, _ in args), name
    for other in (_native.SIGNATURES, _native.ROUTE_SIGNATURES, _native.SOURCE_SIGNATURES):
        assert not set(_native.LEVEL_SIGNATURES) & set(other)  # a table of its own
    # nastar_forward_ex's parameters, in that order, with `levels` where order and order_out were
    ex = _prototypes("nastar.h")["nastar_forward_ex"][1]
    want = [a for a in ex if a[1] not in ("order", "order_out")]
    want.insert([n for _, n in ex].index("order"), ("p", "levels"))
    assert protos["nastar_forward_levels"][1] == want
    assert [n for _, n in protos["nastar_levels_in_launch"][1]] == ["H", "W", "flags", "want_log"]
    assert protos["nastar_placement_slots"][1] == _prototypes("nastar.h")["nastar_placement_from_levels"][1]
    hdr = open(os.path.join(ROOT, "include", "nastar_levels.h")).read()
    assert re.search(r"^#define NASTAR_LEVELS_ABI 1\b", hdr, flags=re.M) and not re.search(r"#define NASTAR_VERSION", hdr)


def test_library_exports_the_level_symbols():
    from neural_astar import _native
    lib = _native.load()
    for sym in _native.LEVEL_SIGNATURES:
        assert hasattr(lib, sym), sym
    assert lib.nastar_levels_abi() == 1
    assert lib.nastar_forward_levels.argtypes is not None and len(lib.nastar_forward_levels.argtypes) == 22


# ---- 3. refusals, made before any HIP call ---------------------------------------------------------------------------------------------
FLAG_UNIT_COST, FLAG_CHECK_ORDER, FLAG_LOCKSTEP, FLAG_MARK_COUPLED = 64, 256, 1024, 32768  # include/nastar.h


def level_args(**over):
    p = 0x10000  # never dereferenced: every call below is refused on its arguments
    a = dict(cost=p, start=p, goal=p, passable=p, B=2, H=32, W=32, g_ratio=0.5, max_iters=1024, histories_out=p, paths_out=p, sel_log_out=None,
             iters_out=p, status_out=p, packed_out=None, workspace=None, workspace_bytes=0, flags=0, levels=p, status_summary=None,
             completion_counter=None, stream=None)
    a.update(over)
    return a


# (what is refused, the return code, nastar_levels_in_launch for the same H, W, flags, want_log)
REFUSALS = [(dict(levels=None), 5, 1), (dict(flags=FLAG_UNIT_COST), 2, 0), (dict(H=20, W=44), 2, 0), (dict(sel_log_out=0x10000), 2, 0),
            (dict(flags=FLAG_LOCKSTEP), 2, 0), (dict(H=90, W=100), 2, 0), (dict(H=32, W=64), 2, 0), (dict(flags=1 << 20), 2, 0),
            (dict(cost=0x10004), 2, 1),  # maps that are not 16-byte aligned have no ranked kernel either (nothing the host-only query can see)
            (dict(cost=None), 5, 1), (dict(B=0), 1, 1)]


@pytest.mark.parametrize("over,rc,in_launch", REFUSALS)
def test_forward_levels_refuses_without_a_device(over, rc, in_launch):
    from neural_astar import _native
    lib = _native.load()
    a = level_args(**over)
    assert lib.nastar_forward_levels(*a.values()) == rc
    assert lib.nastar_levels_in_launch(a["H"], a["W"], a["flags"], int(a["sel_log_out"] is not None)) == in_launch


def test_levels_in_launch_names_the_three_sizes():
    from neural_astar import _native
    lib = _native.load()
    for W in (16, 32, 64):
        assert lib.nastar_levels_in_launch(W, W, 0, 0) == 1 and lib.nastar_levels_in_launch(W, W, FLAG_MARK_COUPLED, 0) == 1
        assert lib.nastar_levels_in_launch(W, W, 0, 1) == 0
        assert _native.forward_levels_address(W, W, 0) != 0 and _native.forward_levels_address(W, W, FLAG_UNIT_COST) == 0
    for H, W in ((8, 8), (20, 44), (128, 128), (0, 0)):
        assert lib.nastar_levels_in_launch(H, W, 0, 0) == 0 and _native.forward_levels_address(H, W, 0) == 0
    assert lib.nastar_placement_slots(None, 4, 0x10000, None) == 5 and lib.nastar_placement_slots(0x10000, 0, 0x10000, None) == 1
