"""CPU: the solvability proof beside the search launch (include/nastar_verdict.h) -- everything that needs no GPU.

1. the seventh header against ``_native.VERDICT_SIGNATURES``; the library exports and binds its symbols; ``nastar.h`` does not change;
2. the refusals of ``nastar_solvable_proof``, made before any HIP call (so they need no device), and ``nastar_solvable_proof_supported``;
3. the switch ``NASTAR_EARLY_VERDICT`` as ``_native.solvable_proof_address`` sees it.
"""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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


# ---- 1. header and binding -----------------------------------------------------------------------------------------------------------
def test_seventh_header_and_verdict_signatures_agree():
    from neural_astar import _native
    protos = _prototypes("nastar_verdict.h")
    assert sorted(protos) == sorted(_native.VERDICT_SIGNATURES) == ["nastar_solvable_proof", "nastar_solvable_proof_supported",
                                                                   "nastar_solvable_proof_sync", "nastar_verdict_abi"]
    for name, (ret, args) in protos.items():
        assert ret == "i", name
        assert _native.VERDICT_SIGNATURES[name] == ret + " " + "".join(k for k, _ in args), name
    for other in (_native.SIGNATURES, _native.ROUTE_SIGNATURES, _native.SOURCE_SIGNATURES, _native.LEVEL_SIGNATURES, _native.FIELD_SIGNATURES,
                  _native.TILED_FIELD_SIGNATURES):
        assert not set(_native.VERDICT_SIGNATURES) & set(other)  # a table of its own
    assert [n for _, n in protos["nastar_solvable_proof"][1]] == ["cost", "start", "goal", "passable", "B", "H", "W", "proved_out", "word", "counter",
                                                                  "stream"]
    hdr = open(os.path.join(ROOT, "include", "nastar_verdict.h")).read()
    assert re.search(r"^#define NASTAR_VERDICT_ABI 1\b", hdr, flags=re.M) and not re.search(r"#define NASTAR_VERSION", hdr)
    assert re.search(r"^#define NASTAR_PROOF_ALL 1\b", hdr, flags=re.M) and re.search(r"^#define NASTAR_PROOF_SOME 2\b", hdr, flags=re.M)


def test_library_exports_and_binds_the_verdict_symbols():
    from neural_astar import _native
    lib = _native.load()
    for sym in _native.VERDICT_SIGNATURES:
        assert hasattr(lib, sym), sym
    assert lib.nastar_verdict_abi() == 1
    assert lib.nastar_solvable_proof.argtypes is not None and len(lib.nastar_solvable_proof.argtypes) == 11
    assert lib.nastar_solvable_proof_sync.argtypes == []


# ---- 2. refusals, made before any HIP call ---------------------------------------------------------------------------------------------
def proof_args(**over):
    p = 0x10000  # never dereferenced: every call below is refused on its arguments
    a = dict(cost=p, start=p, goal=p, passable=p, B=2, H=32, W=32, proved_out=None, word=p, counter=p, stream=None)
    a.update(over)
    return a


# (what is refused, the return code): 5 = NASTAR_ERR_NULL, 1 = NASTAR_ERR_BAD_SHAPE, 2 = NASTAR_ERR_UNSUPPORTED
REFUSALS = [(dict(cost=None), 5), (dict(start=None), 5), (dict(goal=None), 5), (dict(passable=None), 5), (dict(word=None), 5),
            (dict(counter=None), 5), (dict(B=0), 1), (dict(H=0, W=0), 1), (dict(H=16, W=16), 2), (dict(H=20, W=45), 2), (dict(H=32, W=64), 2),
            (dict(H=128, W=128), 2), (dict(cost=0x10004), 2), (dict(goal=0x10008), 2)]


@pytest.mark.parametrize("over,rc", REFUSALS)
def test_solvable_proof_refuses_without_a_device(over, rc):
    from neural_astar import _native
    lib = _native.load()
    assert lib.nastar_solvable_proof(*proof_args(**over).values()) == rc


def test_supported_names_the_two_sizes():
    from neural_astar import _native
    lib = _native.load()
    for H, W, want in ((32, 32, 1), (64, 64, 1), (16, 16, 0), (20, 45, 0), (32, 64, 0), (64, 32, 0), (128, 128, 0), (0, 0, 0)):
        assert lib.nastar_solvable_proof_supported(H, W) == want, (H, W)


# ---- 3. the switch -------------------------------------------------------------------------------------------------------------------
def test_the_switch_turns_the_proof_address_off():
    from neural_astar import _native
    prev = _native.EARLY_VERDICT
    try:
        _native.EARLY_VERDICT = True
        assert _native.solvable_proof_address(32, 32) != 0 and _native.solvable_proof_address(64, 64) == _native.solvable_proof_address(32, 32)
        assert _native.solvable_proof_address(16, 16) == 0 and _native.solvable_proof_address(20, 45) == 0
        _native.EARLY_VERDICT = False
        assert _native.solvable_proof_address(32, 32) == 0
    finally:
        _native.EARLY_VERDICT = prev
    src = open(os.path.join(ROOT, "neural-astar_amd", "neural_astar", "_native.py")).read()
    assert 'os.environ.get("NASTAR_EARLY_VERDICT", "1") != "0"' in src  # read once, at import


def test_the_proof_is_used_only_where_its_cost_bound_covers_the_g_ratio():
    """bound (b) of the header keeps the fixed-point inequality strict in fp32 while 1 - g_ratio >= 0.25"""
    from neural_astar import ops
    assert ops.PROOF_MAX_G_RATIO == 0.75
    for g, want in ((0.5, True), (0.6, True), (0.75, True), (0.7500001, False), (0.9, False), (0.9999, False), (1.0, False), (0.49, False), (0.0, False)):
        assert ops.proof_covers(g) is want, g
        assert not (want and ops.coupling_possible(g))
    hdr = open(os.path.join(ROOT, "include", "nastar_verdict.h")).read()
    src = open(os.path.join(ROOT, "neural-astar_amd", "csrc", "nastar_verdict.hip.h")).read()
    assert "61440 / (H * W)" in hdr and "[0.5, 0.75]" in hdr and re.search(r"kProofMaxRouteCost = 61440\.f;", src)
