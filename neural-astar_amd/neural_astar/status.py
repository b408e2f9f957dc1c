"""What a finished search launch says, read in ONE place (``ops`` re-exports every name): the cells of its status-summary row and
the pinned board they live on, what a row means (``Summary``), when a call runs the exact batch-loop pipeline without waiting for it (``needs_exact``)."""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from . import _native

STATUS_UNSOLVABLE = 3  # NASTAR_ERR_UNSOLVABLE (per-map status)
STATUS_NOT_UNIT_COST = 7  # NASTAR_ERR_NOT_UNIT_COST (per-map status)
STATUS_BAD_HEURISTIC = 8  # NASTAR_ERR_BAD_HEURISTIC (per-map status): a NaN / infinite value in this map's heuristic_maps
SUMMARY_WORDS = 16  # NASTAR_SUMMARY_WORDS
SUMMARY_BAD_ORDER = 15  # NASTAR_SUMMARY_BAD_ORDER
SUMMARY_COUPLED = 14  # NASTAR_SUMMARY_COUPLED: a NOTE (a finished map is not at a fixed point of the reference's batch loop), cells 1..13 are errors
SUMMARY_ERRORS = slice(1, 14)


def coupling_possible(g_ratio: float) -> bool:
    """Can a map that reached its goal fail to be at a fixed point of the reference's batch loop with costs >= 0?
    f(n) - f(goal) = (2 g_ratio - 1) c_goal + (1 - g_ratio)(h0(n) + c_n) is positive for every g_ratio in [0.5, 1): never there.  (With
    NEGATIVE costs any g_ratio can: the launch's status summary reports it, NASTAR_SUMMARY_COUPLED.)"""
    return not (0.5 <= float(g_ratio) < 1.0)


# the largest g_ratio at which forward() relies on the solvability proof (include/nastar_verdict.h): the proof's bound on the costs keeps the
# fixed-point inequality strict in fp32 only while 1 - g_ratio >= 0.25 (csrc/nastar_verdict.hip.h: kProofMaxRouteCost)
PROOF_MAX_G_RATIO = 0.75


def proof_covers(g_ratio: float) -> bool:
    """is "every map ends with status 0 and no summary cell" implied by the solvability proof at this g_ratio?"""
    return 0.5 <= float(g_ratio) <= PROOF_MAX_G_RATIO


_ERROR_BITS = sum(1 << c for c in range(1, 14))  # SUMMARY_ERRORS as bits of the mask csrc/nastar_fastlane.cpp returns (bit c <=> cell c is non-zero)


class Summary(NamedTuple):
    """What a status-summary row says: from the 16 int32 cells as a numpy row (``of_row``; None = a launch that reported nothing) or from the mask
    of cells 1..15 the native host lane returns (``of_bits``).  Cells 1..13 are errors (the per-map status codes), 14 and 15 are notes; errors
    come before the note, which counts only for a batch of more than one map: the call sites ask ``planner.differentiable_astar.deliver``."""
    errors: bool     # some map ended with a per-map status 1..13
    coupled: bool    # NASTAR_SUMMARY_COUPLED as written, whatever the batch size
    bad_order: bool  # NASTAR_SUMMARY_BAD_ORDER: the placement order was no permutation and was ignored (warned about once)
    not_unit: bool   # cell STATUS_NOT_UNIT_COST by itself (one of the errors): InFlightPlanner re-runs such a batch on the general kernel

    @classmethod
    def of_row(cls, row) -> "Summary":
        return CLEAN if row is None else cls(bool(row[SUMMARY_ERRORS].any()), bool(row[SUMMARY_COUPLED]), bool(row[SUMMARY_BAD_ORDER]), bool(row[STATUS_NOT_UNIT_COST]))

    @classmethod
    def of_bits(cls, v: int) -> "Summary":
        return CLEAN if not v else cls(bool(v & _ERROR_BITS), bool(v & (1 << SUMMARY_COUPLED)), bool(v & (1 << SUMMARY_BAD_ORDER)), bool(v & (1 << STATUS_NOT_UNIT_COST)))


CLEAN = Summary(False, False, False, False)


def needs_exact(B: int, g_ratio: float, heuristic: bool = False, unit: bool = False) -> bool:
    """Does this call run marks + lock-step finish up front?  Batch semantics.  For g_ratio in [0.5, 1) with costs >= 0 a
    finished map is at a fixed point of the reference's batch loop and ONE launch is the whole story; the launch reports the rare exception (negative
    costs) in its status summary.  Outside that range the class is reachable with ordinary costs: the exact pipeline runs straight away (marks + three
    launches that do nothing when no map is marked) -- under autograd, with deferred or no checking, inside a hipGraph capture or a trace alike.  With
    a caller's heuristic the class is reachable at every g_ratio (the fixed-point proof needs h0(n) >= 1.001 and h0(goal) = 0); unit costs never are."""
    return B > 1 and (coupling_possible(g_ratio) or heuristic) and not unit


class StatusBoard:
    """Pinned host memory the search launches write their STATUS SUMMARY into (include/nastar.h: status_summary of nastar_forward_ex): one
    row of NASTAR_SUMMARY_WORDS int32 per launch in flight; cell c (1..15) becomes 1 when some map of that launch ended with per-map status
    c, cell 0 when every search of the launch is over (completion_counter: one device cell per row).  "Did any map of this batch fail?" is
    then a poll of one host word and a 64-byte read -- no reduction launch, no device-to-host copy, no stream wait, nothing on a side
    stream.  One board per device; rows are handed out and returned by the callers."""

    _boards: dict = {}

    def __init__(self, device: torch.device, rows: int = 256):
        with torch.cuda.device(device):
            self.t = torch.zeros((rows, SUMMARY_WORDS), dtype=torch.int32).pin_memory()
            self.counters = torch.zeros((rows,), dtype=torch.int32, device=device)
        self.np = self.t.numpy()
        self.base = self.t.data_ptr()
        self.cbase = self.counters.data_ptr()
        self.device = device
        self.free = list(range(rows - 1, -1, -1))
        self.zombies: list = []  # rows whose owner went away before its launch was known to be over (retire()): reaped by acquire()
        self.proved: dict = {}  # zombie rows of launches whose caller returned on the PROOF that every map is solvable -> who that was (retire(proved=...))
        self.lib = _native.load()

    @classmethod
    def of(cls, device: torch.device) -> "StatusBoard":
        key = device.index if device.index is not None else torch.cuda.current_device()
        b = cls._boards.get(key)
        if b is None:
            b = cls._boards[key] = cls(torch.device("cuda", key))
        return b

    def acquire(self) -> int:
        if self.zombies:
            self._reap(False)
        if not self.free and self.zombies:
            self._reap(True)
        if not self.free:
            raise RuntimeError("more than 256 search launches with an unread status: call raise_if_unsolvable() / collect() on the planners that issued them")
        return self.free.pop()

    def retire(self, row: int, event: Optional["torch.cuda.Event"], proved: Optional[str] = None) -> None:
        """give a row back although nobody read it (its planner was dropped with verdicts pending): it is reused only once its launch is over
        -- the completion flag is up, or ``event`` (recorded behind the launch) has passed.  ``proved``: the caller returned early on the proof
        that every map of the launch is solvable (include/nastar_verdict.h) -- a description of the call, for the error message; the launch
        still owns the row until its flag is up, and must then have reported nothing"""
        self.zombies.append((row, event))
        if proved:
            self.proved[row] = proved

    def _reap(self, wait: bool) -> None:
        keep = []
        broken = []  # (row, cells) of launches that reported a status although their batch had been PROVED solvable
        for row, ev in self.zombies:
            if self.np[row, 0] or (ev is not None and ev.query()):
                pass
            elif wait:
                if ev is not None:
                    ev.synchronize()
                else:
                    torch.cuda.synchronize(self.device)
            else:
                keep.append((row, ev))
                continue
            who = self.proved.pop(row, None)
            if who is not None:
                cells = [c for c in range(1, SUMMARY_WORDS) if self.np[row, c]]
                if cells:
                    broken.append((who, row, cells))
            self.release(row)
        self.zombies = keep
        if broken:
            # (raised from whichever call reaps the row: the call it is about returned long ago -- so every one of them is named)
            raise RuntimeError("search launch(es) that the solvability proof (include/nastar_verdict.h) had declared solvable reported a status, and "
                               "the forward() calls that issued them returned WITHOUT raising -- their outputs are suspect: "
                               + "; ".join(f"{who} (status row {row}): summary cell(s) {cells}" for who, row, cells in broken)
                               + ".  Set NASTAR_EARLY_VERDICT=0 and report this")

    def ptr(self, row: int) -> int:
        return self.base + 4 * SUMMARY_WORDS * row

    def counter_ptr(self, row: int) -> int:
        return self.cbase + 4 * row

    def done(self, row: int) -> bool:
        """has the launch that was handed ``ptr(row)`` AND ``counter_ptr(row)`` finished every search?  (one host read)"""
        return bool(self.np[row, 0])

    def wait(self, row: int, stream: Optional["torch.cuda.Stream"] = None, spin_us: int = 2000) -> bool:
        """return once the verdict of the launch that owns ``row`` is complete (True: its completion flag was seen; False: a stream was waited for): poll the completion flag for at most ``spin_us``, then fall
        back to waiting for ``stream`` (default: the device) -- a launch that carried no completion counter (maps larger than LDS) or one
        that takes longer than the spin budget ends up there"""
        if self.np[row, 0] or (spin_us > 0 and self.lib.nastar_host_wait_nonzero(self.ptr(row), spin_us)):
            return True
        if stream is not None:
            stream.synchronize()
        else:
            torch.cuda.synchronize(self.device)
        if spin_us > 0 and not self.np[row, 0]:
            # the launch was given the row's completion counter (callers spin only then) and is over without having raised the flag: an aborted
            # launch left the cell out of phase.  (Launches WITHOUT a counter -- custom-op path, maps larger than LDS -- end up here on every
            # call and must not pay a device write for it: ADVICE r5.)
            self.counters[row] = 0
        return False

    def read(self, row: int):
        """the row as a numpy view if any STATUS cell (1..15) is set, else None (the launch that was handed the row must be over: wait())"""
        r = self.np[row]
        return r if r[1:].any() else None  # (incl. the notes in cells 14 / 15: the caller tells errors -- SUMMARY_ERRORS -- from notes)

    def release(self, row: int) -> None:
        self.np[row] = 0
        self.free.append(row)
