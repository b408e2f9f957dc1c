"""A numpy / Python restatement of the OPEN-LIST BOOKKEEPING of the large-map search (csrc/nastar_forward_hybrid_body.inc), with planted defects.

The CPU oracle (oracle/nastar_oracle.c) scans every cell per step; the kernel never does.  It keeps ``cmin`` -- one (key << 32 | cell) entry
per 64 cells -- and ``smin`` -- one per 4,096 cells, lane ``l`` of the wavefront owning entries ``[l*spl, (l+1)*spl)`` -- and names each step's
next selection as the first-index minimum over FOUR sets it has at hand: the selected cell's chunk without it, the rest of its super-chunk, the
rest of the map, and the neighbours it has just relaxed.  This module restates exactly that, lane by lane, with the oracle's fp32 arithmetic
for the keys (one rounding per operation, IEEE division, the reference's heuristic) and the kernel's multiply-and-correct row division.  It
exists for one purpose: tests/test_hybrid_edges.py plants each ``defect`` below and shows which scenario of tests/hybrid_edges.py notices --
a scenario table that lets a defect through is missing a scenario.

  nbr_super         a relaxed neighbour enters ``cmin`` but not the ``smin`` entry of ANOTHER super-chunk than the selected cell's
  last_entry        the loop over a lane's ``spl`` entries keeps the last of equal keys, not the first
  own_lane          that loop leaves out the selected cell's super-chunk by ``lane == S`` instead of ``lane*spl + j == S``
  pad_open          the padded cells of the last chunk count as open, with key 0
  row_nocorr        the row of a flat index is ``(int)((i + 0.5) * fl(1/W))`` without the correction step
  lock_goal_closed  lock-step mode closes a selected goal like any other cell

``run`` returns (selection log, step count, status); status FAULT (-1) = the restated kernel would have left the map (a selected or relaxed
cell outside ``[0, HW)``), where the emulation stops.
"""
from __future__ import annotations

import math

import numpy as np

f32 = np.float32
KEY_INF = 0xFFFFFFFF
IDLE = (1 << 64) - 1
NO_CELL = 0xFFFFFFFF
FAULT = -1
UNSOLVABLE = 3
DEFECTS = ("nbr_super", "last_entry", "own_lane", "pad_open", "row_nocorr", "lock_goal_closed")
# lane j of 0..7 relaxes the j-th cell of the 3x3 stencil without its centre, in raster order (ascending cells)
DR = np.array([-1, -1, -1, 0, 0, 1, 1, 1], np.int64)
DC = np.array([-1, 0, 1, -1, 1, -1, 0, 1], np.int64)
LANES = np.arange(64, dtype=np.int64)


def _ord(q):
    """fp32 -> u32 whose unsigned order is the floats' order (nastar_device.hip.h f32_to_ord), on arrays"""
    u = np.ascontiguousarray(q, f32).view(np.uint32).astype(np.int64)
    return np.where(u >> 31 != 0, u ^ 0xFFFFFFFF, u ^ 0x80000000)


def _first_min(keys, cells):
    """(minimal key, cell of the FIRST lane holding it): ballot + first set lane + readlane"""
    m = int(keys.min())
    return m, int(cells[int(np.argmax(keys == m))])


class _Map:
    def __init__(self, cost, start, goal, passable, g_ratio, defect):
        assert defect is None or defect in DEFECTS, defect
        self.defect = defect
        self.H, self.W = cost.shape
        self.HW = self.H * self.W
        self.nchunks = (self.HW + 63) // 64
        self.nsuper = (self.nchunks + 63) // 64
        self.spl = (self.nsuper + 63) // 64
        HWp = self.nchunks * 64
        self.cost = np.ascontiguousarray(cost, f32).reshape(-1)
        self.gr, self.omg = f32(g_ratio), f32(1.0 - g_ratio)
        self.sqrtW = f32(math.sqrt(self.W))
        self.inv_W = f32(1.0) / f32(self.W)
        self.g = np.full(HWp, -np.inf, f32)  # +inf passable and never opened, -inf closed / obstacle / padding, finite = open
        self.g[:self.HW][passable.reshape(-1) != 0] = np.inf
        self.cmin = [IDLE] * (self.nsuper * 64)
        self.smin = [IDLE] * (self.spl * 64)
        s, g = np.flatnonzero(start.reshape(-1)), np.flatnonzero(goal.reshape(-1))
        self.sidx = int(s[-1]) if s.size else -1  # the fill launch's atomicMax: the LAST non-zero cell
        self.gidx = int(g[-1]) if g.size else -1
        self.goal_r, self.goal_c = (int(x[0]) for x in self.row(np.array([max(self.gidx, 0)], np.int64)))

    # -- arithmetic -------------------------------------------------------------------------------------------------------
    def row(self, i):
        """hybrid_row / hybrid_row_nb on an array of flat indices -> (rows, columns)"""
        r = ((i.astype(f32) + f32(0.5)) * self.inv_W).astype(np.int64)  # (i < 2^21: exact in fp32; truncation = floor)
        c = i - r * self.W
        if self.defect != "row_nocorr":
            lo, hi = c < 0, c >= self.W
            r = np.where(lo, r - 1, np.where(hi, r + 1, r))
            c = np.where(lo, c + self.W, np.where(hi, c - self.W, c))
        return r, c

    def h0(self, r, c):
        """get_heuristic, one fp32 rounding per operation (oracle/nastar_oracle.c heuristic0)"""
        a, b = r.astype(f32) - f32(self.goal_r), c.astype(f32) - f32(self.goal_c)
        dr, dc = np.abs(a), np.abs(b)
        cheb = (dr + dc) - np.minimum(dr, dc)
        return cheb + f32(0.001) * np.sqrt(a * a + b * b)

    def key(self, g, h):
        """ordered key of q = fl(fl(fl(g_ratio g) + fl((1 - g_ratio) h)) / fl32(sqrt(W))), h = fl(h0 + cost)"""
        with np.errstate(invalid="ignore"):
            return _ord((self.gr * g + self.omg * h) / self.sqrtW)

    # -- the search ---------------------------------------------------------------------------------------------------------
    def run(self, budget, lock):
        log = []
        if self.sidx < 0 or self.gidx < 0:
            return log, 0, UNSOLVABLE
        d, spl, W, HW = self.defect, self.spl, self.W, self.HW
        sr, sc = self.row(np.array([self.sidx], np.int64))
        k0 = int(self.key(f32(0.0), self.h0(sr, sc) + self.cost[self.sidx])[0])
        self.g[self.sidx] = 0.0
        self.cmin[self.sidx >> 6] = self.smin[self.sidx >> 12] = (k0 << 32) | self.sidx
        sel_cell = self.sidx
        status = 0
        while len(log) < budget:
            s = sel_cell
            if s == NO_CELL:
                status = UNSOLVABLE
                break
            log.append(s)
            if s >= HW:
                return log, len(log), FAULT
            at_goal = s == self.gidx
            if at_goal and not lock:
                break
            stay = lock and at_goal and d != "lock_goal_closed"  # lock-step: a selected goal is expanded and stays on the open list
            C, S = s >> 6, s >> 12
            # the rest of the map: every lane's entries but the one of S, the first minimal one of each lane, then the first minimal lane
            eE = []
            for lane in range(64):
                e0 = IDLE
                for j in range(spl):
                    own = (lane == S) if d == "own_lane" else (lane * spl + j == S)
                    ej = IDLE if own else self.smin[lane * spl + j]
                    if j == 0 or ((ej >> 32) <= (e0 >> 32) if d == "last_entry" else (ej >> 32) < (e0 >> 32)):
                        e0 = ej
                eE.append(e0)
            mE, cE = _first_min(np.array([e >> 32 for e in eE], np.int64), np.array([e & NO_CELL for e in eE], np.int64))
            # the rest of the super-chunk of s: its 64 chunk entries but the one of C
            ev = self.cmin[S * 64:S * 64 + 64]
            kS = np.array([KEY_INF if lane == (C & 63) else e >> 32 for lane, e in enumerate(ev)], np.int64)
            mS, cS = _first_min(kS, np.array([e & NO_CELL for e in ev], np.int64))
            # neighbours (lanes 0..7) and the chunk of s (64 lanes): one round trip's loads
            r, c = self.row(np.array([s], np.int64))
            nr, nc = r + DR, c + DC
            inb = (nr >= 0) & (nr < self.H) & (nc >= 0) & (nc < W)
            n = np.where(inb, s + DR * W + DC, s)
            if ((n < 0) | (n >= HW)).any():
                return log, len(log), FAULT
            ic = C * 64 + LANES
            icv = ic < HW
            ics = np.where(icv, ic, 0)
            gs, gn, gc = self.g[s], self.g[n], self.g[ic]
            cs, cn, cc = self.cost[s], self.cost[n], self.cost[ics]
            hn = self.h0(nr, nc)
            hc = self.h0(*self.row(ics))
            g2 = gs + cs
            upd = inb & (gn > g2)
            open_c = icv & np.isfinite(gc) & ((ic != s) | stay)
            kn = np.where(upd, self.key(g2, hn + cn), KEY_INF)
            kc = np.where(open_c, self.key(gc, hc + cc), KEY_INF)
            if d == "pad_open":
                kc = np.where(icv, kc, 0)
            mC, cC = _first_min(kc, ic)
            mN, cN = _first_min(kn, n)
            # stores
            if not stay:
                self.g[s] = -np.inf
            self.g[n[upd]] = g2
            # open list: the chunk and super-chunk of s by plain writes, the neighbours by minimum into both levels
            kCS = min(mC, mS)
            cCS = min(cC if mC == kCS else NO_CELL, cS if mS == kCS else NO_CELL)
            self.cmin[C] = IDLE if mC == KEY_INF else (mC << 32) | cC
            self.smin[S] = IDLE if kCS == KEY_INF else (kCS << 32) | cCS
            for k, cell in zip(kn[upd], n[upd]):
                en = (int(k) << 32) | int(cell)
                self.cmin[cell >> 6] = min(self.cmin[cell >> 6], en)
                if not (d == "nbr_super" and (cell >> 12) != S):
                    self.smin[cell >> 12] = min(self.smin[cell >> 12], en)
            # the next selection
            kX = min(mE, mN)
            cX = min(cE if mE == kX else NO_CELL, cN if mN == kX else NO_CELL)
            sel_key = min(kCS, kX)
            sel_cell = min(cCS if kCS == sel_key else NO_CELL, cX if kX == sel_key else NO_CELL)
            if sel_key == KEY_INF:
                sel_cell = NO_CELL
        return log, len(log), status


def run(cost, start, goal, passable, g_ratio, max_iters, defect=None, lock_steps=None):
    """one map ([H,W] arrays) -> (selection log as an int32 array, steps, status).  ``lock_steps``: lock-step mode for exactly that many steps
    (the FINAL launch of the batch-loop finish); None: the search stops at the step that selects its goal, or at ``max_iters``."""
    m = _Map(np.asarray(cost), np.asarray(start), np.asarray(goal), np.asarray(passable), g_ratio, defect)
    log, iters, status = m.run(max_iters if lock_steps is None else lock_steps, lock_steps is not None)
    return np.asarray(log, np.int32), iters, status
