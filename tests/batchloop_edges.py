"""The cases of tests/test_batchloop_edges.py (CPU) and tests/test_batchloop_edges_gpu.py (GPU): the exact batch loop (DESIGN.md section 2.3;
nastar_forward_batchloop_finish: PROBE, nastar_batchloop_tend_kernel, FINAL) at the batch sizes, bitmap words and budgets at which its code
takes another path, and the CPU oracle's answers for them.  Importable without a device; nothing here reads a kernel's output.

Vocabulary.  ``sm``: every map searched alone (oracle mode "sm"); ``d``: the reference's literal batch loop (mode "dense").
``tmax = sm.iters.max() - 1`` over the maps that take part: the last own goal step.  ``t_end = d.t_batch``: the step that ends the batch loop.
A map ``wanders`` in a pool when the pool's batch run selects something else than its goal right after its own goal step: such a map is not at
a fixed point of the loop, the early-exit launch marks it, and in any batch that runs past its goal step its histories differ from ``sm``.

Classes (one GPU test function each):
  A  large batches: the stride ``b += 1024`` of the tend kernel over maps and over marked maps, its LDS AND over (long long)B * nw words
  B  bit and word seams of the probe bitmap and of the tend kernel (w0 = tmax >> 5, the mask of word 0, t_end in a later word)
  C  budgets that end the loop (the clamp t_end = max_iters - 1, the partial last bitmap word)
  D  long budgets: the LDS branch of the tend kernel at its largest launch, the first budget of the global branch, 600000 steps
  E  maps that take no part (a walled-in goal, an empty start map) inside a large batch
  F  the masked and the heuristic finish entry points at B >= 1025

The sub-batches of classes B, C and D are map indices into a seeded pool, found by ``find_seams`` (the oracle alone, seeded) and committed
below as SEAMS; ``python tests/batchloop_edges.py`` prints the table again.  tests/test_batchloop_edges.py holds every case to the predicate of
its class, so a generator that drifts fails there, on the CPU.
"""
from __future__ import annotations

import functools
import itertools
from typing import NamedTuple, Optional, Tuple

import numpy as np

MOORE8 = 0x1EF
VON_NEUMANN = 0x0AA
STATUS_UNSOLVABLE = 3
TEND_THREADS = 1024      # csrc/nastar_search_kernels.hip.h kTendThreads: the stride of the tend kernel's loops
TEND_LDS_WORDS = 16380   # kTendMaxLdsWords: the most bitmap words the tend kernel ANDs in LDS (its own 16 bytes + these stay within 64 KiB)
OLD_LDS_WORDS = 16384    # the limit before the cap: exactly 64 KiB of dynamic LDS beside the kernel's own cells

# name -> (maps, H, W, g_ratio, kind).  kind: "plain" costs U(0, 10); "zero30" the same with about 30 % zero-cost cells; "signed" costs
# U(-2.5, 7.5) (costs below -1); "vn" plain, only the maps the von Neumann neighbourhood solves
POOLS = {
    "p8": (1100, 8, 8, 0.2, "plain"),
    "p16": (2100, 16, 16, 0.2, "plain"),
    "p12": (600, 12, 12, 0.0, "plain"),
    "z16": (600, 16, 16, 1.0, "zero30"),
    "s16": (1025, 16, 16, 0.5, "signed"),
    "p32": (1025, 32, 32, 0.2, "plain"),
    "p80": (6, 80, 80, 0.2, "plain"),
    "v12": (1100, 12, 12, 0.0, "vn"),
    "h12": (1100, 12, 12, 0.5, "zero30"),
}


class Pool(NamedTuple):
    cost: np.ndarray      # [N,H,W] float32
    start: np.ndarray
    goal: np.ndarray
    passable: np.ndarray
    g_ratio: float


def _freeze(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def pool(name: str) -> Pool:
    from neural_astar.utils import synthetic as syn
    from oracle import oracle as O
    N, H, W, g_ratio, kind = POOLS[name]
    n_gen = 2 * N if kind == "vn" else N
    pr = syn.random_obstacle_maps(n_gen, H, W, 0.2, 3)
    if kind == "signed":
        cost = syn.random_costs(n_gen, H, W, 4, lo=-2.5, hi=7.5)
    else:
        cost = syn.random_costs(n_gen, H, W, 4, hi=10.0)
    if kind == "zero30":
        cost = np.where(np.random.Generator(np.random.PCG64(5)).random(cost.shape) < 0.3, np.float32(0), cost).astype(np.float32)
    arrays = [np.ascontiguousarray(a[:, 0]) for a in (cost, pr.start_maps, pr.goal_maps, pr.map_designs)]
    if kind == "vn":
        st = O.forward(*arrays, g_ratio, W * W, mode="sm", neighbor_mask=VON_NEUMANN).map_status
        keep = np.flatnonzero(st == 0)[:N]
        assert keep.size == N, (name, keep.size)
        arrays = [np.ascontiguousarray(a[keep]) for a in arrays]
    _freeze(*arrays)
    return Pool(*arrays, g_ratio)


class Case(NamedTuple):
    name: str
    cls: str                         # "A" .. "F"
    pool: str
    maps: Tuple[int, ...]            # pool indices, in batch order
    max_iters: Optional[int] = None  # None: W * W (eval mode)
    want_log: bool = True
    seam: str = ""                   # class B / D: the predicate of SEAM_PREDICATES / the branch the case claims
    nw: int = 0                      # class D: words - (tmax >> 5) the case claims (0: none)
    walled: Tuple[int, ...] = ()     # class E: batch positions whose goal is walled in (status 3)
    no_start: Tuple[int, ...] = ()   # class E: batch positions with an all-zero start map (status 3)
    mask: Optional[int] = None       # class F: the neighbourhood (None: the entry points without a mask)
    zero_h: bool = False             # class F: caller heuristic maps of zeros

    @property
    def shape(self):
        return POOLS[self.pool][1:3]

    @property
    def budget(self) -> int:
        return self.max_iters if self.max_iters is not None else self.shape[1] ** 2

    @property
    def g_ratio(self) -> float:
        return POOLS[self.pool][3]


class Inputs(NamedTuple):
    cost: np.ndarray
    start: np.ndarray
    goal: np.ndarray
    passable: np.ndarray
    h0: Optional[np.ndarray]


class Expected(NamedTuple):
    """the oracle's answers for a case, [B, ...] over the whole batch; rows of maps that take no part hold the state machine's (``sm``) values"""
    ok: np.ndarray         # [B] bool: the map takes part in the batch loop
    hist: np.ndarray       # d.histories
    paths: np.ndarray      # d.paths
    log: Optional[np.ndarray]  # d.sel_log [B, max_iters] (-1 past the loop's end), None without want_log
    t_end: int             # d.t_batch
    tmax: int
    sm_hist: np.ndarray
    sm_paths: np.ndarray
    sm_iters: np.ndarray
    sm_log: Optional[np.ndarray]
    sm_status: np.ndarray  # [B] 0 / 3; -1 where the oracle has no answer (an empty start map)

    @property
    def differs(self) -> np.ndarray:
        """[B] bool: the batch run of the map is not the map alone"""
        return self.ok & (self.hist != self.sm_hist).any((1, 2))


def inputs(c: Case) -> Inputs:
    p = pool(c.pool)
    idx = np.asarray(c.maps, np.int64)
    cost, start, goal, passable = (np.ascontiguousarray(a[idx]) for a in p[:4])
    H, W = c.shape
    for b in c.walled:
        r0, c0 = (int(v) for v in np.argwhere(goal[b])[0])
        for dr in (-1, 0, 1):
            for dc in (-1, 0, 1):
                if (dr or dc) and 0 <= r0 + dr < H and 0 <= c0 + dc < W:
                    passable[b, r0 + dr, c0 + dc] = 0
    for b in c.no_start:
        start[b] = 0
    return Inputs(cost, start, goal, passable, np.zeros_like(cost) if c.zero_h else None)


def _oracle_pair(c: Case, x: Inputs, rows: np.ndarray):
    """(sm, d as (hist, paths, log, t_end)) of the rows `rows` of the batch; ``sm`` also covers the walled-in maps among them"""
    from oracle import oracle as O
    a = [np.ascontiguousarray(v[rows]) for v in x[:4]]
    T = c.budget
    if c.zero_h:
        import heuristic_oracle as HO
        mask = MOORE8 if c.mask is None else c.mask
        s = HO.search(*a, x.h0[rows], c.g_ratio, T, mask, lockstep=False)
        d = HO.search(*a, x.h0[rows], c.g_ratio, T, mask, lockstep=True)

        def log_of(r):
            out = np.full((len(rows), T), -1, np.int32)
            for b, sel in enumerate(r.sel):
                out[b, :len(sel)] = sel
            return out
        return (s.histories, s.paths, s.iters, log_of(s) if c.want_log else None, s.status), \
               (d.histories, d.paths, log_of(d) if c.want_log else None, d.t_batch)
    kw = {} if c.mask is None else {"neighbor_mask": c.mask}
    s = O.forward(*a, c.g_ratio, T, mode="sm", want_log=c.want_log, **kw)
    return (s.histories, s.paths, s.iters, s.sel_log, s.map_status), None


@functools.lru_cache(maxsize=None)
def expected(c: Case) -> Expected:
    from oracle import oracle as O
    x = inputs(c)
    B = len(c.maps)
    T = c.budget
    searched = np.setdiff1d(np.arange(B), np.asarray(c.no_start, np.int64))  # the maps the oracle has an answer for
    (sh, sp, si, sl, ss), dd = _oracle_pair(c, x, searched)
    sm_hist = np.zeros((B,) + c.shape, np.float32)
    sm_paths = np.zeros((B,) + c.shape, np.int64)
    sm_iters = np.zeros(B, np.int32)
    sm_status = np.full(B, -1, np.int32)
    sm_log = np.full((B, T), -1, np.int32) if c.want_log else None
    sm_hist[searched], sm_paths[searched], sm_iters[searched], sm_status[searched] = sh, sp, si, ss
    if c.want_log:
        sm_log[searched] = sl
    ok = sm_status == 0
    rows = np.flatnonzero(ok)
    if dd is None or rows.size != searched.size:
        a = [np.ascontiguousarray(v[rows]) for v in x[:4]]
        if c.zero_h:
            _, dd = _oracle_pair(c, x, rows)
        else:
            d = O.forward(*a, c.g_ratio, T, mode="dense", want_log=c.want_log, **({} if c.mask is None else {"neighbor_mask": c.mask}))
            assert d.status == 0, (c.name, d.status)
            dd = (d.histories, d.paths, d.sel_log, d.t_batch)
    hist, paths = sm_hist.copy(), sm_paths.copy()
    hist[rows], paths[rows] = dd[0], dd[1]
    log = None
    if c.want_log:
        log = sm_log.copy()
        log[rows] = dd[2]
    e = Expected(ok, hist, paths, log, int(dd[3]), int(sm_iters[ok].max()) - 1, sm_hist, sm_paths, sm_iters, sm_log, sm_status)
    _freeze(*(v for v in e if isinstance(v, np.ndarray)))
    return e


# ---- which maps of a pool wander -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pool_runs(name: str):
    """(sm.iters, wanders [N] bool, differs [N] bool) of the whole pool run as one batch"""
    from oracle import oracle as O
    p = pool(name)
    N, H, W = p.cost.shape
    sm = O.forward(*p[:4], p.g_ratio, W * W, mode="sm")
    d = O.forward(*p[:4], p.g_ratio, W * W, mode="dense", want_log=True)
    assert d.status == 0 and (sm.map_status == 0).all(), name
    gi = p.goal.reshape(N, -1).argmax(1)
    nxt = np.minimum(sm.iters, d.t_batch)  # the step after the map's own goal step (the pool's slowest maps have none: they do not count)
    wanders = (sm.iters <= d.t_batch) & (d.sel_log[np.arange(N), nxt] != gi)
    differs = (d.histories != sm.histories).any((1, 2))
    _freeze(wanders, differs)
    return sm.iters, wanders, differs


# ---- the seam classes: predicates on (tmax, t_end, every map wanders, some map differs) ----------------------------------------------------
SEAM_PREDICATES = {
    "tmax_bit0": lambda tmax, t_end, differs: tmax & 31 == 0 and tmax >= 32 and differs,
    "tmax_bit31": lambda tmax, t_end, differs: tmax & 31 == 31 and differs,
    "tend_same_word": lambda tmax, t_end, differs: t_end > tmax and t_end >> 5 == tmax >> 5 and tmax >= 32,
    "tend_later_word": lambda tmax, t_end, differs: t_end >> 5 > tmax >> 5,
    "tend_is_tmax": lambda tmax, t_end, differs: t_end == tmax and differs,
    "w0_zero": lambda tmax, t_end, differs: tmax < 32 and differs,
}
C_BUDGETS = (20, 31, 32, 33, 64, 65)


def _sub_batch(name: str, maps):
    """(tmax, t_end, some map differs) of the sub-batch `maps` of pool `name` at the eval budget"""
    from oracle import oracle as O
    p = pool(name)
    idx = np.asarray(maps, np.int64)
    a = [np.ascontiguousarray(v[idx]) for v in p[:4]]
    W = p.cost.shape[-1]
    d = O.forward(*a, p.g_ratio, W * W, mode="dense")
    sm = O.forward(*a, p.g_ratio, W * W, mode="sm")
    return int(sm.iters.max()) - 1, int(d.t_batch), bool((d.histories != sm.histories).any())


def find_seams(seed: int = 11, tries: int = 4000):
    """the seeded search behind SEAMS: sub-batches of 2-5 wandering maps per predicate (pool p16; w0_zero: p8), the class-C batch (three
    wandering maps that finish early and two slow ones of p16: its natural t_end lies beyond every budget of C_BUDGETS) and the class-D
    batches (three maps of p12 whose loop runs past tmax; two of p80 one of which wanders)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    found = {}
    for pred, pname in [(k, "p8" if k == "w0_zero" else "p16") for k in SEAM_PREDICATES]:
        iters, wanders, _ = pool_runs(pname)
        cand = np.flatnonzero(wanders)
        for _ in range(tries):
            maps = tuple(int(v) for v in rng.choice(cand, int(rng.integers(2, 6)), replace=False))
            if SEAM_PREDICATES[pred](*_sub_batch(pname, maps)):
                found[pred] = (pname, maps)
                break
    iters, wanders, _ = pool_runs("p16")
    quick, slow = np.flatnonzero(wanders & (iters <= 15)), np.flatnonzero(iters >= 80)
    for _ in range(tries):
        maps = tuple(int(v) for v in np.concatenate([rng.choice(quick, 3, replace=False), rng.choice(slow, 2, replace=False)]))
        if _sub_batch("p16", maps)[1] >= max(C_BUDGETS) + 2:
            found["C"] = ("p16", maps)
            break
    iters, wanders, _ = pool_runs("p12")
    for _ in range(tries):
        maps = tuple(int(v) for v in rng.choice(len(iters), 3, replace=False))
        tmax, t_end, differs = _sub_batch("p12", maps)
        if differs and t_end > tmax:
            found["D12"] = ("p12", maps)
            break
    for maps in itertools.combinations(range(POOLS["p80"][0]), 2):  # (six maps: the first pair with a map that wanders)
        if _sub_batch("p80", maps)[2]:
            found["D80"] = ("p80", maps)
            break
    return found


# find_seams(11): key -> (pool, map indices)
SEAMS = {
    "tmax_bit0": ("p16", (124, 1785, 51, 1021, 1426)),
    "tmax_bit31": ("p16", (1863, 1227, 330, 153, 1810)),
    "tend_same_word": ("p16", (1060, 1021)),
    "tend_later_word": ("p16", (1451, 1788, 307, 1842, 515)),
    "tend_is_tmax": ("p16", (633, 829)),
    "w0_zero": ("p8", (631, 366, 532, 1097, 798)),
    "C": ("p16", (2099, 1316, 904, 1330, 1913)),
    "D12": ("p12", (500, 414, 402)),
    "D80": ("p80", (3, 4)),
}


# ---- the table -----------------------------------------------------------------------------------------------------------------------------
def _long_budget(pname, maps, nw):
    """the budget whose probe bitmap has exactly `nw` words from word tmax >> 5 on, with a partial last word"""
    tmax = int(pool_runs(pname)[0][list(maps)].max()) - 1
    return 32 * (nw + (tmax >> 5)) - 5


def _spread(n_maps, count, seed, exclude=()):
    """`count` batch positions, half of them below TEND_THREADS and half at or above it (seeded)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    lo = [int(v) for v in rng.permutation(TEND_THREADS) if v not in exclude][:count - count // 2]
    hi = [int(v) for v in TEND_THREADS + rng.permutation(n_maps - TEND_THREADS) if v not in exclude][:count // 2]
    return tuple(sorted(lo + hi))


@functools.lru_cache(maxsize=None)
def table():
    """name -> Case, in table order"""
    rows = []

    def tiled(pname, B):
        """the pool, repeated up to B maps; a batch of 1025 ends with a copy of the pool's first wandering map: the one map behind the stride
        of the tend kernel is a marked one"""
        maps = np.arange(B) % POOLS[pname][0]
        if B == TEND_THREADS + 1 and pname != "h12":
            maps[-1] = np.flatnonzero(pool_runs(pname)[1])[0]
        return tuple(int(v) for v in maps)

    # A: large batches
    rows += [Case("A_8x8_1025", "A", "p8", tiled("p8", 1025)), Case("A_8x8_2100", "A", "p8", tiled("p8", 2100)),
             Case("A_8x8_4096", "A", "p8", tiled("p8", 4096)),
             Case("A_12x12_2100", "A", "p12", tiled("p12", 2100)), Case("A_16x16_1025", "A", "p16", tiled("p16", 1025)),
             Case("A_16x16_2100", "A", "p16", tiled("p16", 2100)), Case("A_16x16_4096", "A", "p16", tiled("p16", 4096)),
             Case("A_16x16_zero_cost_1025", "A", "z16", tiled("z16", 1025)), Case("A_16x16_signed_1025", "A", "s16", tiled("s16", 1025)),
             Case("A_32x32_1025", "A", "p32", tiled("p32", 1025))]
    # more than 1024 MARKED maps: the pool's wandering maps, repeated, in front of and between the others
    w = np.flatnonzero(pool_runs("p8")[1])
    rest = np.flatnonzero(~pool_runs("p8")[1])[:200]
    many = np.concatenate([np.tile(w, -(-1100 // w.size))[:1100], rest])
    many = many[np.random.Generator(np.random.PCG64(7)).permutation(many.size)]
    rows.append(Case("A_8x8_marked_1100", "A", "p8", tuple(int(v) for v in many)))
    # the ONLY marked maps behind the stride, and t_end behind tmax: 1024 fixed points that finish no later than the seam case's slowest map,
    # then that case's maps -- the maps behind index 1024 alone decide how many maps are marked and where the loop ends
    pname, sub = SEAMS["tend_later_word"]
    iters, wanders, _ = pool_runs(pname)
    fill = np.flatnonzero(~wanders & (iters <= iters[list(sub)].max()))
    front = np.tile(fill, -(-TEND_THREADS // fill.size))[:TEND_THREADS]
    rows.append(Case("A_16x16_marked_behind_1024", "A", pname, tuple(int(v) for v in front) + tuple(sub)))
    # B: seams
    for pred in SEAM_PREDICATES:
        pname, maps = SEAMS[pred]
        rows.append(Case(f"B_{pred}", "B", pname, maps, seam=pred))
    # C: budgets
    pname, maps = SEAMS["C"]
    rows += [Case(f"C_budget_{t}", "C", pname, maps, max_iters=t) for t in C_BUDGETS]
    # D: long budgets
    pname, maps = SEAMS["D12"]
    rows += [Case(f"D_12x12_nw{nw}", "D", pname, maps, max_iters=_long_budget(pname, maps, nw), want_log=False, nw=nw, seam=seam)
             for nw, seam in ((TEND_LDS_WORDS, "lds"), (TEND_LDS_WORDS + 1, "global"), (OLD_LDS_WORDS, "global"), (OLD_LDS_WORDS + 1, "global"))]
    rows.append(Case("D_12x12_600000", "D", pname, maps, max_iters=600000, want_log=False, seam="global"))
    pname, maps = SEAMS["D80"]
    rows.append(Case("D_80x80_600000", "D", pname, maps, max_iters=600000, want_log=False, seam="global"))
    # E: maps that take no part, the slowest map of the batch among them
    for name, pname, B in (("E_8x8_1100", "p8", 1100), ("E_16x16_2100", "p16", 2100)):
        iters = pool_runs(pname)[0]
        slowest = int(np.argmax(iters[:B]))
        p = pool(pname)
        sr, sc = np.divmod(p.start.reshape(len(iters), -1).argmax(1), p.cost.shape[-1])
        gr, gc = np.divmod(p.goal.reshape(len(iters), -1).argmax(1), p.cost.shape[-1])
        near = tuple(int(v) for v in np.flatnonzero(np.maximum(abs(sr - gr), abs(sc - gc))[:B] <= 1))  # (a start beside its goal needs no free cell)
        walled = tuple(sorted((slowest,) + _spread(B, B // 50, 13, exclude=(slowest,) + near)))
        rows.append(Case(name, "E", pname, tiled(pname, B), walled=walled, no_start=_spread(B, 4, 17, exclude=walled)))
    # F: the other finish entry points
    rows.append(Case("F_masked_12x12_1100", "F", "v12", tiled("v12", 1100), mask=VON_NEUMANN))
    rows.append(Case("F_heuristic_12x12_1025", "F", "h12", tiled("h12", 1025), zero_h=True))
    assert len({r.name for r in rows}) == len(rows)
    return {r.name: r for r in rows}


def cases(cls: str):
    return [c for c in table().values() if c.cls == cls]


def names(cls: str):
    """the case names of a class WITHOUT building the table's pools (pytest ids at collection time)"""
    return _NAMES[cls]


_NAMES = {
    "A": ["A_8x8_1025", "A_8x8_2100", "A_8x8_4096", "A_12x12_2100", "A_16x16_1025", "A_16x16_2100", "A_16x16_4096", "A_16x16_zero_cost_1025",
          "A_16x16_signed_1025", "A_32x32_1025", "A_8x8_marked_1100", "A_16x16_marked_behind_1024"],
    "B": [f"B_{k}" for k in SEAM_PREDICATES],
    "C": [f"C_budget_{t}" for t in C_BUDGETS],
    "D": [f"D_12x12_nw{n}" for n in (TEND_LDS_WORDS, TEND_LDS_WORDS + 1, OLD_LDS_WORDS, OLD_LDS_WORDS + 1)] + ["D_12x12_600000", "D_80x80_600000"],
    "E": ["E_8x8_1100", "E_16x16_2100"],
    "F": ["F_masked_12x12_1100", "F_heuristic_12x12_1025"],
}


if __name__ == "__main__":
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(root, "neural-astar_amd"), root, os.path.join(root, "tests")]
    for k, v in find_seams().items():
        print(f'    "{k}": {v!r},')
