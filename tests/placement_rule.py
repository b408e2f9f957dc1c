"""numpy restatement of the in-launch placement rule (include/nastar_levels.h, csrc/nastar_placement.hip.h: ranked_map) -- test helper.

nblk = ceil(B / 64); block j holds the maps j, j + nblk, j + 2 nblk, ... below B; workgroup i = r * nblk + j searches the member of block j
with exactly r members ahead of it: larger clamp(level, 0, 4095) first, the lower map first among equals.  Written as a stable sort per
block -- the device code finds the same member by a bit descent over packed keys, so the two share the rule and nothing else.
"""
import numpy as np

MAX_LEVEL = 4095
BATCH_SIZES = (1, 2, 63, 64, 65, 130, 4096, 4097)  # one map, a partial only block, the 64 / 65 edge, a partial last row of two-plus blocks


def slots(levels) -> np.ndarray:
    """order[i] = the map workgroup i searches"""
    lv = np.clip(np.asarray(levels).astype(np.int64).reshape(-1), 0, MAX_LEVEL)
    B = lv.size
    nblk = (B + 63) // 64
    out = np.full(B, -1, np.int32)
    for j in range(nblk):
        members = np.arange(j, B, nblk)
        assert members.size <= 64
        ranked = members[np.argsort(-lv[members], kind="stable")]
        out[j + np.arange(members.size) * nblk] = ranked
    return out


def is_permutation(order, B) -> bool:
    o = np.asarray(order).reshape(-1)
    return o.size == B and np.array_equal(np.sort(o), np.arange(B))


def level_sets(B, seed=0):
    """the level sets of the tests: {name: int32 [B]}"""
    rng = np.random.default_rng(seed + B)
    wild = rng.integers(-50, 6000, B).astype(np.int64)
    wild[::7] = np.iinfo(np.int32).max
    wild[3::11] = np.iinfo(np.int32).min
    wild[5::13] = MAX_LEVEL + 1
    return {
        "random_with_ties": rng.integers(0, 12, B).astype(np.int32),
        "all_equal": np.full(B, 17, np.int32),
        "ascending": np.arange(B, dtype=np.int32),
        "descending": np.arange(B, dtype=np.int32)[::-1].copy(),
        "out_of_range": wild.astype(np.int32),
    }
