"""``DifferentiableAstar`` -- host shim over the HIP search kernel.

Mirrors the public surface of the reference module (``planner/differentiable_astar.py``): ``AstarOutput``
(:16-23), ``DifferentiableAstar(g_ratio, Tmax)`` (:128-148) with the ``neighbor_filter`` parameter kept for
state-dict compatibility (:140-143), and ``forward(cost_maps, start_maps, goal_maps, obstacles_maps,
store_intermediate_results)`` (:150-267).  The body of the reference's loop is NOT here: it is
``csrc/nastar_search.hip.h`` reached through ``torch.ops.nastar.astar_forward``.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional

import torch
import torch.nn as nn

from .. import _native, ops
from ..status import Summary, needs_exact


class AstarOutput(NamedTuple):
    """Output structure of A* search planners (same fields/order as the reference, :16-23)."""

    histories: torch.Tensor
    paths: torch.Tensor
    intermediate_results: Optional[List[dict]] = None


class RoutedAstarOutput(NamedTuple):
    """What ``plan_routes()`` returns: the two masks of ``AstarOutput`` and, per map, the ORDERED route they cannot give (with 8-connected
    moves a path cell may have more than two path neighbours).  ``routes`` [B, L] int32: flat cell indices r*W + c in travel order, the goal
    last, then -1 (``route_coords`` turns them into (row, col)); ``route_lengths`` [B] int32: the number of route cells (== paths.sum per
    map), the true length also when L is smaller -- the row then holds the LAST L cells; ``route_costs`` [B] float32: the cost of the cells
    the route leaves (every cell but the goal), summed in float64 and rounded once.  DESIGN.md section 2, item 6c."""

    histories: torch.Tensor
    paths: torch.Tensor
    routes: torch.Tensor
    route_lengths: torch.Tensor
    route_costs: torch.Tensor


FieldOutput = ops.FieldOutput  # what ``cost_to_go()`` returns (dists, policies, status): DESIGN.md section 2, item 6e
PathOutput = ops.PathOutput  # what ``shortest_paths()`` returns (paths, costs, status): DESIGN.md section 2, item 6j


class FieldRoutesOutput(NamedTuple):
    """What ``plan_many()`` returns: ``dists`` [B,1,H,W], the cost-to-go field the routes were read off, the four tensors of
    ``ops.FieldRoutes`` -- ``routes`` [B,S,L] int32, ``route_lengths``, ``route_costs`` and ``status`` [B,S] -- and ``paths`` [B,S,H,W]
    int64, the 0/1 mask of the cells ``routes`` holds, or None.  DESIGN.md section 2, item 6i."""

    dists: torch.Tensor
    routes: torch.Tensor
    route_lengths: torch.Tensor
    route_costs: torch.Tensor
    status: torch.Tensor
    paths: Optional[torch.Tensor] = None


def route_coords(routes: torch.Tensor, W: int) -> torch.Tensor:
    """``routes`` [B, L] (flat indices r*W + c, -1 = no cell) -> [B, L, 2] (row, col), -1 where the route is -1"""
    none = routes < 0
    idx = routes.clamp(min=0)
    rc = torch.stack((torch.div(idx, W, rounding_mode="floor"), idx % W), dim=-1)
    return rc.masked_fill(none.unsqueeze(-1), -1)


def _checked_route_len(max_route_len) -> Optional[int]:
    """``max_route_len`` of plan_routes(): None (the capacity that always suffices) or an int >= 1"""
    if max_route_len is None:
        return None
    if isinstance(max_route_len, bool) or not isinstance(max_route_len, int) or max_route_len < 1:
        raise ValueError(f"max_route_len must be an int >= 1 (or None: min(H*W, max_iters + 1), which always suffices), got {max_route_len!r}")
    return max_route_len


# ---- the reference module's public helpers, kept importable under their names (differentiable_astar.py:26-52, :77-93, :96-125) -------------
# The search kernel fuses all three (a-2, a-4, a-7 of SURVEY.md 8a): nothing in this package calls them.  They exist for code that imports them
# from the reference's module -- same arguments, same results -- and work on device tensors (no CPU path in this package).

def get_heuristic(goal_maps: torch.Tensor, tb_factor: float = 0.001) -> torch.Tensor:
    """Chebyshev distance + ``tb_factor`` x Euclidean distance to the one-hot goal of every map (reference :26-52), same shape as ``goal_maps``.
    The default ``tb_factor`` runs the ``nastar_heuristic`` kernel (bit-exact with the reference's fp32 arithmetic, tests/test_gpu_parity.py);
    any other factor is the same sequence of fp32 operations as device tensor ops."""
    ops._require_device(goal_maps)
    if float(tb_factor) == 0.001 and goal_maps.dtype == torch.float32:
        return ops.heuristic(goal_maps)
    B, H, W = goal_maps.shape[0], goal_maps.shape[-2], goal_maps.shape[-1]
    flat = goal_maps.reshape(B, H * W)
    rows = torch.arange(H, device=goal_maps.device).repeat_interleave(W).to(goal_maps.dtype)
    cols = torch.arange(W, device=goal_maps.device).repeat(H).to(goal_maps.dtype)
    gr, gc = flat @ rows, flat @ cols                                # (one-hot goal maps: the goal's row / column)
    dr, dc = rows[None, :] - gr[:, None], cols[None, :] - gc[:, None]
    ar, ac = dr.abs(), dc.abs()
    cheb = (ar + ac) - torch.minimum(ar, ac)
    return (cheb + tb_factor * torch.sqrt(dr * dr + dc * dc)).reshape(goal_maps.shape)


def expand(x: torch.Tensor, neighbor_filter: torch.Tensor) -> torch.Tensor:
    """The 8-neighbourhood of the selected nodes ``x`` [B,H,W]: one grouped 3x3 convolution with zero padding (reference :77-93;
    ``neighbor_filter`` [B,1,3,3], ``DifferentiableAstar.neighbor_filter`` repeated per map)."""
    ops._require_device(x)
    y = torch.nn.functional.conv2d(x[None], neighbor_filter, padding=1, groups=x.shape[0])
    return y.squeeze().squeeze(0)  # (the reference's squeezes: a batch of one comes back as [H,W])


def backtrack(start_maps: torch.Tensor, goal_maps: torch.Tensor, parents: torch.Tensor, current_t: int) -> torch.Tensor:
    """Path maps (int64, shape of ``goal_maps``) from a parent table [B,HW]: the goal, then ``current_t`` hops along ``parents`` starting at the
    goal's parent, every visited cell marked (reference :96-125; like it, the walk does not stop at the start -- the initial table points every cell
    at the goal, so it re-walks cells it has marked)."""
    ops._require_device(parents)
    B = parents.shape[0]
    par = parents.to(torch.long).reshape(B, -1)
    path = goal_maps.to(torch.long).clone()
    flat = path.view(B, -1)
    loc = (par * flat).sum(-1, keepdim=True)                          # the goal's parent
    one = torch.ones_like(loc)
    for _ in range(int(current_t)):
        flat.scatter_(1, loc, one)
        loc = par.gather(1, loc)
    return path


class UnsolvableMapError(RuntimeError):
    """Raised (when ``check_solvable``) for maps whose goal is unreachable.

    The reference produces NaNs and then an ``IndexError`` inside ``backtrack`` for the whole batch
    (SURVEY.md section 0.4); here the kernel reports a per-map status instead."""


class _PendingStatus:
    """status of an earlier launch on its way to the host: the launch itself writes its summary -- and, when every search is over, its
    completion flag -- into a pinned ``ops.StatusBoard`` row.  Nothing is recorded, copied or launched for it: ``done()`` is one host
    read; ``stream`` is only the fall-back for launches that carry no completion counter (maps larger than LDS)."""

    def __init__(self, status: torch.Tensor, row: int, seq: int = 0, flagged: bool = True, repair=None):
        self.status = status
        self.seq = seq
        self.row = row
        self.repair = repair  # callable or None: completes a launch that reported NASTAR_SUMMARY_COUPLED to the reference's batch loop, in place
        self.board = ops.StatusBoard.of(status.device)
        self.stream = torch.cuda.current_stream(status.device)
        self.event = None
        self.released = False
        if not flagged:
            self.event = torch.cuda.Event()
            self.event.record(self.stream)

    def done(self) -> bool:
        return self.board.done(self.row) if self.event is None else self.event.query()

    def raise_if_unsolvable(self) -> None:
        if self.event is None:
            self.board.wait(self.row, self.stream)  # (flagged launch: spins on the completion flag first)
        else:
            self.event.synchronize()
        summ = Summary.of_row(self.board.read(self.row))
        self.board.release(self.row)
        self.released = True
        repair, self.repair = self.repair, None
        if deliver(summ, self.status, self.seq, deferred=True) and repair is not None:
            repair()

    def __del__(self):  # a planner dropped with verdicts pending: the row goes back once its launch is over (never while it may still be written)
        try:
            if not self.released:
                self.released = True
                self.board.retire(self.row, self.event)
        except Exception:  # noqa: BLE001 -- interpreter shutdown
            pass


def _capturing(t: torch.Tensor) -> bool:
    """is a hipGraph capture underway on the stream this tensor's work goes to?  (CPU tensors: no -- the op itself rejects them)"""
    return t.is_cuda and torch.cuda.is_current_stream_capturing()


def _raise_unsolvable(status: torch.Tensor, seq: int = 0, deferred: bool = False) -> None:
    nu = torch.nonzero(status == ops.STATUS_NOT_UNIT_COST).flatten().tolist()
    if nu:
        raise ValueError(f"unit_cost=True, but {len(nu)} map(s) hold values other than 0.0 / 1.0 (batch rows {nu[:16]}"
                         f"{'...' if len(nu) > 16 else ''} of search call #{seq}): their outputs are empty; use unit_cost='auto' or False")
    bh = torch.nonzero(status == ops.STATUS_BAD_HEURISTIC).flatten().tolist()
    if bh:
        raise ValueError(f"non-finite heuristic: heuristic_maps of {len(bh)} map(s) hold a NaN or an infinite value (batch rows {bh[:16]}"
                         f"{'...' if len(bh) > 16 else ''} of search call #{seq}): those maps were not searched, the others were")
    bad = torch.nonzero(status != 0).flatten().tolist()
    where = f"search call #{seq} of this module" + (" (an EARLIER call: check_solvable='deferred' delivers verdicts late)" if deferred else "")
    raise UnsolvableMapError(
        f"{len(bad)} map(s) have no start->goal route or a non-one-hot start/goal map "
        f"(batch rows {bad[:16]}{'...' if len(bad) > 16 else ''} of {where})")


def deliver(summary: Summary, status: torch.Tensor, seq: int, deferred: bool = False) -> bool:
    """What the ``Summary`` of search call #``seq`` means to its caller, in this order: warn (once) about an ignored placement order; raise for an error
    cell; True = the launch reported NASTAR_SUMMARY_COUPLED for a batch of more than one map (the caller runs the batch again, exactly)."""
    if summary.bad_order:
        _warn_bad_order()
    if summary.errors:
        _raise_unsolvable(status, seq, deferred)
    return summary.coupled and status.numel() > 1


def _same_tensor(a: torch.Tensor, b: torch.Tensor) -> bool:
    """are the cost map and the obstacle map ONE tensor?  (VanillaAstar hands one over as both, reference astar.py:93-94: the kernel then loads it once)"""
    return a is b or (a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.stride() == b.stride())


class Placement:
    """Memory of ONE batch that truly recurs (a fixed evaluation set held in memory -- same maps AND same start cells at every visit): the
    order in which its searches finished at the previous visit.  ``planner.astar.placement = p`` before a call makes that call start the
    longest searches first (``order`` / ``order_out`` of ``nastar_forward_ex``, include/nastar.h) and leaves the order for the next visit
    in ``p`` -- no extra launch, no host synchronisation, identical outputs.  The first visit (or a visit with another batch size) runs in
    the natural order -- unless the batch carries its loader's hint (``start_maps.placement_order``, ``ops.OrderHint``), which always takes
    precedence: the reference's loaders re-draw every start cell at every visit (utils/data.py:152-166), so for THEIR batches only the
    hint describes the searches at hand."""

    def __init__(self):
        self.bufs: Optional[List[torch.Tensor]] = None
        self.k = 0            # bufs[k] holds the order of the latest visit
        self.valid = False    # ... once one visit has run

    def buffers(self, B: int, device) -> "tuple[Optional[torch.Tensor], torch.Tensor]":
        """(order to use now or None, buffer that receives the order of this visit).  Nothing changes until ``commit()``: a call that
        fails before its launch must not leave a half-initialised order behind for the next visit."""
        if self.bufs is None or self.bufs[0].numel() != B + 1 or self.bufs[0].device != device:
            self.bufs = [ops.new_placement_buffer(B, device) for _ in range(2)]
            self.k, self.valid = 0, False
        return (self.bufs[self.k] if self.valid else None), self.bufs[self.k ^ 1]

    def commit(self) -> None:
        """the launch that was handed ``buffers()`` has been issued: its output buffer is the order of the latest visit"""
        self.k ^= 1
        self.valid = True

    def __getstate__(self):  # device scratch is not state (deepcopy / pickle of a planner that holds one)
        return {"bufs": None, "k": 0, "valid": False}


class DifferentiableAstar(nn.Module):
    def __init__(self, g_ratio: float = 0.5, Tmax: float = 1.0, check_solvable=True, unit_cost="auto"):
        """
        Args:
            g_ratio: weight of g(v) in f = g_ratio*g + (1-g_ratio)*h; 0 = best-first search (reference :129-135).
            Tmax: fraction of W*W search steps allowed in training mode (reference :135,:200-202).
            check_solvable: what to do about maps whose open list ran empty (extension over the reference, which crashes with an
                ``IndexError`` inside ``backtrack`` for the whole batch):
                ``True`` / ``"sync"`` (default) -- wait for the kernel and raise ``UnsolvableMapError`` IN THE SAME CALL, before
                the caller can consume garbage histories or step an optimiser on them (one device->host sync per call: ~27 us on
                a 4096-map 32x32 batch; the reference synchronises once per search ITERATION);
                ``"deferred"`` (opt-in: benchmarks, pipelined inference loops) -- NO host synchronisation in ``forward()``: the
                per-map status travels to the host asynchronously (a device-side any() + a copy into pinned memory + an event)
                and the error is raised by the first LATER ``forward()`` call that finds the verdict already on the host, or by
                ``raise_if_unsolvable()``, which waits (call it after the last batch / before consuming results); the message
                names the call it belongs to;
                ``False`` -- never raise.  Inside a hipGraph capture nothing is checked (nothing may synchronise there).
                The per-map status of the latest call is always available as ``self.last_status``.
                BATCH SEMANTICS are exact in every mode for costs >= 0: a ``g_ratio`` outside [0.5, 1) -- where a map that reached its goal
                may not be at a fixed point of the reference's batch loop -- runs the exact pipeline (``ops._launch_search``: marks + lock-step
                re-run of the marked maps, no host round trip); inside [0.5, 1) only NEGATIVE costs can do that: the same-call verdict
                re-runs such a batch, a deferred verdict completes the outputs in place when it is delivered (or raises, under autograd), and
                ``False`` -- which reads nothing back -- is then each map as if searched alone (the one documented gap).
            unit_cost: the UNIT-COST search kernel (``NASTAR_FLAG_UNIT_COST``, csrc/nastar_search_unit.hip.h) for calls in which
                the cost map and the obstacle map are ONE tensor -- ``VanillaAstar.forward`` (reference astar.py:93-94) -- and no
                gradient or selection log is wanted.  On binary maps every cell the search can touch then costs 1.0, the LDS state
                needs no cost word, and 29 instead of 16 maps of 32x32 are resident per CU: same outputs, ~1.5x the maps/s with
                SEVERAL batches in flight.  One launch at a time is a serial chain that gains nothing from the layout, so
                ``forward()`` takes it only with ``True`` (the kernel CHECKS the promise per map; a map that breaks it raises
                ``ValueError``, with "deferred" checking possibly from a later call); ``"auto"`` (default) and ``False`` run the
                general kernel here.  ``parallel.InFlightPlanner`` is where "auto" means unit-cost first (with a re-run of the
                rare non-binary batch at collection).
        """
        super().__init__()
        nf = torch.ones(1, 1, 3, 3)
        nf[0, 0, 1, 1] = 0
        # the search neighbourhood (reference :140-143, both expand() calls of every step convolve with it): forward() hands it to the kernels as
        # a 9-bit mask (neighbor_mask()); the default filter keeps the Moore-8 kernels
        self.neighbor_filter = nn.Parameter(nf, requires_grad=False)
        self._nf_key = self._filter_key()
        self._nf_mask: Optional[int] = None  # None = Moore-8
        # the reference keeps its heuristic as an INSTANCE attribute (:143), i.e. as something a user may replace; the kernels compute that
        # function (Chebyshev + 0.001 Euclidean) themselves or take the heuristic as a TENSOR (forward(..., heuristic_maps=)): forward()
        # refuses, loudly, to run with anything else in this attribute
        self.get_heuristic = get_heuristic
        self.g_ratio = g_ratio
        assert (Tmax > 0) & (Tmax <= 1), "Tmax must be within (0, 1]"
        self.Tmax = Tmax
        self.check_solvable = check_solvable
        self.unit_cost = unit_cost
        # MULTI-SOURCE search (extension; the reference does it with any multi-hot ``start_maps``: its open list begins as open_maps = start_maps):
        # False (default) = forward() / plan_routes() as they were in every respect -- of several non-zero cells in a start map the kernels
        # take the one with the HIGHEST flat index and say nothing; True = every non-zero cell is a source, open with g = 0 when the search
        # begins, and the path ends at whichever source reached the goal.  An attribute, not a keyword of
        # forward(): the reference's positional calls and the trailing ``heuristic_maps`` keep their places.
        self.multi_source = False
        # collation of sharded steps (parallel.BucketedCollator): a contiguous uint8 tensor [B, 2 * ceil(HW / 8)] the NEXT call's search launch
        # writes its bit-packed masks into (2 bits per cell; fused into the launch for 32x32 / 64x64 maps).  `last_packed` is that tensor when
        # the call did fill it (the checked no-grad call through the native host lane), None otherwise (the collator then packs the outputs itself)
        self.packed_sink = None
        self.last_packed = None
        self.last_status: Optional[torch.Tensor] = None
        self.last_iters: Optional[torch.Tensor] = None
        # how the same-call verdict of the latest checked call reached the host: "proof" (the batch was proved solvable beside its search,
        # include/nastar_verdict.h: forward() returned while the searches were still running), "flag" (the launch's completion flag was seen
        # in pinned memory) or "sync" (a stream was waited for); None before the first such call
        self.last_verdict_source: Optional[str] = None
        self._pending: List[_PendingStatus] = []
        self._calls = 0  # searches launched through this module (names the call in UnsolvableMapError)
        # placement memory of the batch the NEXT forward() searches (see Placement); consumed by that call
        self.placement: Optional[Placement] = None

    # ---- the neighbourhood: neighbor_filter -> the kernels' 9-bit mask ----------------------------------------------------------------------
    def _filter_key(self):
        f = self.neighbor_filter
        return (id(f), f.data_ptr(), f.device, f._version) if f is not None else None

    def neighbor_mask(self) -> Optional[int]:
        """The search neighbourhood of ``neighbor_filter`` as the kernels take it (include/nastar.h NASTAR_NEIGHBORS_*): bit r*3+c <=> filter cell
        (r, c) is 1; None for the default Moore-8 filter (the unmasked kernels).  expand() is conv2d, a cross-correlation: filter cell (a, b) opens
        the neighbour at offset (1-a, 1-b) of the selected cell.  Supported: a [1,1,3,3] filter with weights in {0, 1} and a zero centre (any other
        weight blends g-values and parent indices in the reference -- not a search); anything else raises NotImplementedError.

        Reading a filter that lives on the device is a host synchronisation, so the mask is cached, keyed on the tensor's identity, data_ptr,
        device and version counter, and re-read only when one of them changes: load_state_dict, copy_ / fill_ under no_grad, a new Parameter and
        .to() / .cuda() (which keep the values: no read at all) are all seen.  NOT seen: in-place edits through ``.data`` (torch does not
        version them) -- assign through ``with torch.no_grad(): neighbor_filter.copy_(...)`` instead.  Inside a hipGraph capture or a
        torch.compile trace the cached mask is used as it is, and a filter that changed since it was cached (or was never read) raises.
        What was captured or traced keeps the mask it was captured / traced with: a graph replayed, or a compiled function called again,
        after the filter changed still searches the old neighbourhood (capture or compile again after changing the filter)."""
        key = self._filter_key()
        if key == self._nf_key:
            return self._nf_mask
        f = self.neighbor_filter
        if torch.compiler.is_compiling() or (f is not None and f.is_cuda and torch.cuda.is_current_stream_capturing()):
            raise RuntimeError("DifferentiableAstar.neighbor_filter changed since its mask was last read (or was never read), and reading "
                               "it now -- a host synchronisation -- is impossible inside a hipGraph capture / torch.compile trace: call "
                               "forward() once outside the capture / trace after changing the filter")
        mask = _filter_mask(f)  # raises for an unsupported filter (nothing cached: every call raises)
        self._nf_key, self._nf_mask = key, (None if mask == ops.NEIGHBORS_MOORE8 else mask)
        return self._nf_mask

    def _apply(self, fn, *args, **kwargs):
        # .to() / .cuda() / .half() move or cast the filter without changing its 0 / 1 values: carry a valid cached mask over (no device read)
        valid = self._nf_key is not None and self._nf_key == self._filter_key()
        out = super()._apply(fn, *args, **kwargs)
        if valid:
            self._nf_key = self._filter_key()
        return out

    # run-time bookkeeping (device events, pinned flags, the latest status tensors) is not module state: copy.deepcopy(planner)
    # (EMA / best-model snapshots), pickling and torch.save(planner) must work after any forward()
    def __getstate__(self):
        state = dict(self.__dict__)
        state["_pending"] = []
        state["last_status"] = None
        state["last_iters"] = None
        state["placement"] = None
        return state

    def __setstate__(self, state):
        super().__setstate__(state)
        self.__dict__.setdefault("_pending", [])
        self.__dict__.setdefault("_calls", 0)
        self.__dict__.setdefault("placement", None)
        self.__dict__.setdefault("_nf_mask", None)
        self.__dict__.setdefault("multi_source", False)
        self.__dict__.setdefault("last_verdict_source", None)
        self._nf_key = None  # (a new process / a copied tensor: read the filter again on first use)

    def raise_if_unsolvable(self, wait: bool = True) -> None:
        """Deliver the deferred verdicts: raise ``UnsolvableMapError`` if an earlier ``forward()`` call met an unsolvable map.
        ``wait=True`` (explicit calls) waits for every outstanding launch; ``wait=False`` (what ``forward()`` does) only looks at
        verdicts that have already reached the host."""
        while self._pending and (wait or self._pending[0].done()):
            self._pending.pop(0).raise_if_unsolvable()

    # ---- status protocol of ONE search launch: row = begin_launch(); launch(..., summary_ptr=summary_ptr(row)); note_status(..., row=row) ----
    def begin_launch(self, like: torch.Tensor) -> int:
        """Reserve the pinned status-summary row the next search launch of this module writes into (``ops.StatusBoard``); -1 when
        nothing will be checked (``check_solvable`` False, or a hipGraph capture is underway: nothing may synchronise there)."""
        if not self.check_solvable or not like.is_cuda or _capturing(like):
            return -1
        return ops.StatusBoard.of(like.device).acquire()

    @staticmethod
    def summary_ptr(row: int, like: torch.Tensor) -> int:
        return ops.StatusBoard.of(like.device).ptr(row) if row >= 0 else 0

    def _collect_sync(self, row: int, device: torch.device, flagged: bool = False) -> Summary:
        """wait for the launch that owns ``row``, hand the row back and return what it said (``CLEAN`` = every map ended with status 0);
        ``flagged``: the launch was given the row's completion counter"""
        board = ops.StatusBoard.of(device)
        # the ONE device->host wait of a checked call: a poll of the launch's completion flag in pinned memory (no stream wait, no driver
        # wake-up; the outputs themselves stay stream-ordered), falling back to the stream for launches without a completion counter
        self.last_verdict_source = "flag" if board.wait(row, torch.cuda.current_stream(device), 2000 if flagged else 0) else "sync"
        summ = Summary.of_row(board.read(row))
        board.release(row)
        return summ

    def note_status(self, status: torch.Tensor, iters: torch.Tensor, row: int = -1, flagged: bool = False, repair=None) -> bool:
        """record a launch's per-map status / step counts and apply the ``check_solvable`` policy (also used by the fused training step, which
        launches the search itself).  ``row``: the ``begin_launch()`` row whose address the launch was given as ``summary_ptr`` (``flagged``: and the
        row's completion counter) -- the verdict is then a poll of the row's completion flag (unflagged: a stream wait / an event) and one 64-byte
        host read; without a row the status tensor is reduced on the device (one more launch + a blocking copy).  Returns ``deliver()``'s answer when
        the verdict was read in THIS call: True = the caller runs the batch again with ``exact=True`` (the reference's batch loop to the letter,
        ``ops._launch_search``).  ``repair``: what a DEFERRED verdict that reports the note calls to do the same in place (``_repair_in_place``)."""
        self.last_status, self.last_iters = status, iters
        self._calls += 1
        mode = self.check_solvable
        if not mode or _capturing(status) or torch.compiler.is_compiling():  # nothing may synchronise inside a hipGraph capture / a trace
            if row >= 0:
                ops.StatusBoard.of(status.device).release(row)
            return False
        if mode != "deferred":  # True / "sync": the verdict belongs to THIS call
            if row >= 0:
                return deliver(self._collect_sync(row, status.device, flagged), status, self._calls)
            self.last_verdict_source = "sync"  # (no row: the status tensor itself is read, a blocking copy)
            if bool((status != 0).any()):
                _raise_unsolvable(status, self._calls)
            return False
        if row < 0:  # a launch that carried no summary: reduce on the device into a fresh row's worth of pinned memory
            row = ops.StatusBoard.of(status.device).acquire()
            ops.StatusBoard.of(status.device).t[row, ops.STATUS_UNSOLVABLE:ops.STATUS_UNSOLVABLE + 1].copy_((status != 0).any().reshape(1), non_blocking=True)
            flagged = False
        self._pending.append(_PendingStatus(status, row, self._calls, flagged, repair))
        if len(self._pending) > 64:  # a caller that never lets the device catch up: bound the queue (one wait)
            self._pending.pop(0).raise_if_unsolvable()
        return False

    def exact_search(self, cost_maps, start_maps, goal_maps, passable, max_iters, want_log=False, out_4d=True, neighbor_mask=-1, multi_source=False):
        """The reference's batch loop to the letter for a batch in which a finished map is NOT at a fixed point (NASTAR_SUMMARY_COUPLED;
        DESIGN.md section 2.3): every map of the class is stepped, goal selections included, until the first step at which ALL maps of the
        batch select their goal (reference :219-225, :251) or the budget ends -- the search launch with marks + nastar_forward_batchloop_finish
        (include/nastar.h), any map size, no host round trip.  -> (histories, paths, iters, status, sel_log).  ``neighbor_mask``: -1 = this
        module's (``neighbor_mask()``)"""
        nmask = self.neighbor_mask() if neighbor_mask == -1 else neighbor_mask
        return ops.search_nograd(cost_maps, start_maps, goal_maps, passable, self.g_ratio, max_iters, want_log, out_4d=out_4d, exact=True,
                                 neighbor_mask=nmask, multi_source=multi_source)

    def _repair_in_place(self, inputs, outputs, max_iters, want_log, neighbor_mask=None, multi_source=False):
        """for a DEFERRED verdict: the launch it belongs to reported the note after its outputs had been handed out -- run the exact search now
        and overwrite those tensors (histories, paths, iters, status, sel_log) before the caller, who asked for the verdict first, reads them"""
        import weakref
        # weak references only: a verdict still pending must not keep the outputs of a pipelined loop (48 MB per 4096-map call, up to 64 calls
        # deep) or its inputs alive -- outputs nobody holds any more need no repair
        ins = [weakref.ref(t) for t in inputs]
        outs = [weakref.ref(t) if t is not None else None for t in outputs]

        def repair():
            live = [(r() if r is not None else None) for r in outs]
            if all(t is None for t in live):
                return
            src = [r() for r in ins]
            if any(t is None for t in src):
                raise RuntimeError("a batch searched with check_solvable='deferred' holds a map that is not at a fixed point of the reference's batch loop "
                                   "(negative costs), and its inputs were released before the verdict was collected: the outputs still alive are those of "
                                   "each map searched alone.  Keep the inputs until raise_if_unsolvable(), or use check_solvable=True (DESIGN.md section 2.3)")
            new = self.exact_search(*src, max_iters, want_log, out_4d=False, neighbor_mask=neighbor_mask, multi_source=multi_source)
            for old, fresh in zip(live, new):
                if old is not None and fresh is not None and old.numel() == fresh.numel():
                    old.data.copy_(fresh.reshape(old.shape))
        return repair

    def resolve_placement(self, B: int, start_maps: torch.Tensor, in_lds: bool):
        """(order, order_out, check_order, placement) for the next launch.  The ``OrderHint`` the batch's loader attached to ``start_maps``
        (``start_maps.placement_order``: by the optimal distance of THIS batch's start cells, data the sample carries) comes first -- the
        reference's loaders draw new start cells at every visit of a map (utils/data.py:152-166), so only a hint describes the batch at
        hand; without one, the module's ``placement`` (a batch that really recurs: the order its searches finished in last time).  A
        ``placement`` still records this launch's completion order either way."""
        pl, self.placement = self.placement, None
        if not in_lds:
            return None, None, False, None
        order = order_out = None
        check = False
        prev = None
        if pl is not None:
            prev, order_out = pl.buffers(B, start_maps.device)
        hint = getattr(start_maps, "placement_order", None)
        if hint is not None:
            o = hint.resolve() if isinstance(hint, ops.OrderHint) else hint
            if torch.is_tensor(o) and o.numel() == B and o.device == start_maps.device and o.dtype == torch.int32:
                order, check = o.reshape(-1), not getattr(hint, "trusted", False)
        if order is None and prev is not None:
            order = prev[:B]
        return order, order_out, check, pl

    def _forward_fast(self, cost_maps, start_maps, goal_maps, obstacles_maps) -> Optional[AstarOutput]:
        """The common call -- no gradient, default checking, an LDS-resident size, nothing tracing or capturing -- with its host side in native
        code (csrc/nastar_fastlane.cpp: output allocation, nastar_forward_ex, the poll of the launch's completion flag).  None = not a call for
        this lane (the general path below takes it and raises whatever needs raising).  Same launch, same outputs, same verdict policy."""
        fl = _native.load_fastlane()
        if fl is None:
            return None
        B, _, H, W = cost_maps.shape
        dev = cost_maps.device
        if (not cost_maps.is_cuda or not ops.in_lds(H, W) or needs_exact(B, self.g_ratio) or torch.compiler.is_compiling()
                or torch.cuda.is_current_stream_capturing() or dev.index != torch.cuda.current_device()):
            return None
        same = obstacles_maps is cost_maps
        flags = ops.FLAG_UNIT_COST if (same and self.unit_cost is True) else 0
        flags |= ops.FORWARD_FLAGS
        order = order_out = pl = levels = None
        ws_bytes = 0
        hint = getattr(start_maps, "placement_order", None)
        if (self.placement is None and type(hint) is ops.OrderHint and hint.order is None and hint.levels is not None and hint.levels.numel() == B
                and hint.levels.device == dev):
            # the loader's levels: the search launch ranks them itself where it has a kernel for that (16x16, 32x32, 64x64 on the hand-scheduled
            # streams: include/nastar_levels.h), else the native call sorts them into a placement right in front of the search launch
            levels = hint.levels
        elif self.placement is not None or hint is not None:
            order, order_out, check_order, pl = self.resolve_placement(B, start_maps, True)
            if order is not None and check_order:
                flags |= ops.FLAG_CHECK_ORDER
                ws_bytes = 16
        max_iters = ops.max_iters_for(W, self.Tmax, self.training)
        # EARLY VERDICT (include/nastar_verdict.h): for this launch "every map ends with status 0 and no summary cell" is a property of the inputs
        # alone -- Moore-8, the built-in heuristic, one source (this lane), the general kernel with no flag at all (no order to check, none of
        # the development switches of NASTAR_FORWARD_FLAGS: nothing was proved about those streams), a g_ratio at which a finished map is
        # at a fixed point of the batch loop IN FP32 for every cost the proof accepts (ops.proof_covers: [0.5, 0.75]), a budget no search can
        # exhaust -- and there is a proof kernel for the size
        proof_fn = 0
        if flags == 0 and ops.proof_covers(self.g_ratio) and max_iters >= H * W:
            proof_fn = _native.solvable_proof_address(H, W)
        sink = self.packed_sink  # (a collation slot: the search launch emits the 2-bit-per-cell masks itself, include/nastar.h: packed_out)
        board = ops.StatusBoard.of(dev)
        row = board.acquire()
        prow = -1
        try:
            prow = board.acquire() if proof_fn else -1  # the proof's own row: word + completion counter
            hist, paths, iters, status, _, rc, verdict, proof = fl[0].search(
                fl[1], cost_maps, start_maps, goal_maps, None if same else obstacles_maps, float(self.g_ratio),
                max_iters, False, flags, order, order_out, ws_bytes, board.ptr(row), board.counter_ptr(row),
                torch._C._cuda_getCurrentRawStream(dev.index), 2000, levels, fl[2], sink,
                0 if levels is None else _native.forward_levels_address(H, W, flags),
                proof_fn, board.ptr(prow) if proof_fn else 0, board.counter_ptr(prow) if proof_fn else 0,
                _native.forward_proved_address() if proof_fn else 0)  # (search + proof from one entry point: include/nastar_ticket.h)
        except BaseException:
            board.release(row)
            if prow >= 0:
                board.release(prow)
            raise
        if prow >= 0:
            if proof == 3:
                # the proof's word did not come up within the spin budget: its launch may still read the inputs and owns its row -- wait for it
                _native.check(_native.load().nastar_solvable_proof_sync(), "nastar_solvable_proof_sync")
                board.counters[prow] = 0  # (a launch that ended without its word left the cell out of phase)
                board.release(prow)
            else:
                board.free.append(prow)  # (not launched, or its word was read and zeroed: the row came back clean)
        if rc:
            board.release(row)
            if rc == -1:
                return None  # (strided / mistyped inputs: the general path copies or complains)
            _native.check(rc, "nastar_forward_ex")
        if pl is not None and order_out is not None:
            pl.commit()
        self.last_status, self.last_iters = status, iters
        self._calls += 1
        self.last_packed = sink
        if proof == 1:
            # every map is PROVED solvable: the verdict is 0 whenever the searches end.  They are still running and their launch owns the row
            # until its completion flag is up: the board reaps it then (and checks that the launch indeed reported nothing)
            board.retire(row, None, proved=f"search call #{self._calls} of a {type(self).__name__} at {id(self):#x} ({B} maps of {H}x{W})")
            self.last_verdict_source = "proof"
            return AstarOutput(hist, paths, [])
        self.last_verdict_source = "flag"
        if verdict == 0:  # every map ended with status 0 (the row came back zeroed)
            board.free.append(row)
            return AstarOutput(hist, paths, [])
        if verdict < 0:  # the flag did not come up within the spin budget (a very long launch): wait for the stream, read the row
            summ = self._collect_sync(row, dev, True)
        else:
            board.free.append(row)
            summ = Summary.of_bits(verdict)
        if deliver(summ, status, self._calls):
            # a finished map of this batch is not at a fixed point of the reference's batch loop (negative costs): the batch again, exactly
            hist, paths, iters, status, _ = self.exact_search(cost_maps, start_maps, goal_maps, cost_maps if same else obstacles_maps,
                                                              max_iters, neighbor_mask=None)
            self.last_status, self.last_iters = status, iters
            self.last_packed = None  # (the slot holds the masks of the first launch)
        return AstarOutput(hist, paths, [])

    def _refuse_replaced_heuristic(self) -> None:
        if self.get_heuristic is not get_heuristic:
            raise NotImplementedError("DifferentiableAstar.get_heuristic was replaced: the MI355X search kernels hard-wire the reference's heuristic "
                                      "(Chebyshev + 0.001 x Euclidean, differentiable_astar.py:26-52) and would silently ignore another one; "
                                      "pass the heuristic as a tensor instead: forward(..., heuristic_maps=h0) with h0 of shape [B, 1, H, W]")

    def plan_routes(self, cost_maps: torch.Tensor, start_maps: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor,
                    heuristic_maps: Optional[torch.Tensor] = None, max_route_len: Optional[int] = None) -> RoutedAstarOutput:
        """The search of ``forward()`` -- same kernels, ``histories`` and ``paths`` bit-identical to its -- that also returns every map's ORDERED
        route, its length and its cost (``RoutedAstarOutput``; the launch of include/nastar_routes.h writes them from the parent chain it
        backtracks along).  An EVALUATION call: it runs without an autograd graph and returns detached tensors, whatever requires a gradient.
        Honours ``neighbor_filter``, ``g_ratio``, ``Tmax`` / ``self.training``, ``unit_cost``, ``heuristic_maps`` and the exact batch-loop rule
        of ``forward()`` (a launch that reports NASTAR_SUMMARY_COUPLED is repeated exactly).  ``check_solvable`` False: nothing is checked;
        any other value: the status is read before returning (one host synchronisation) and ``UnsolvableMapError`` raised as ``forward()``
        does.  ``max_route_len``: the row length L of ``routes``; None = min(H*W, max_iters + 1), which always suffices; a shorter row keeps
        the last L cells of a longer route.  Takes no placement and no native host lane.  With ``self.multi_source`` every non-zero cell of
        ``start_maps`` is a source: the route begins at the source that reached the goal (``routes[b, 0]`` when it fits the row) and may pass
        through another start cell; False takes the highest-index start cell only."""
        assert cost_maps.ndim == start_maps.ndim == goal_maps.ndim == obstacles_maps.ndim == 4
        route_cap = _checked_route_len(max_route_len)
        self._refuse_replaced_heuristic()
        h0 = _checked_heuristic(heuristic_maps, cost_maps).detach() if heuristic_maps is not None else None
        ops._require_device(cost_maps, start_maps, goal_maps, obstacles_maps)
        nmask = self.neighbor_mask()
        B, _, H, W = cost_maps.shape
        max_iters = ops.max_iters_for(W, self.Tmax, self.training)
        same = _same_tensor(cost_maps, obstacles_maps)
        multi = bool(self.multi_source)
        unit = same and self.unit_cost is True and nmask is None and h0 is None and not multi
        exact = needs_exact(B, self.g_ratio, h0 is not None, unit)
        dev = cost_maps.device
        cost = cost_maps.detach()
        passable = cost if same else obstacles_maps.detach()
        start, goal = start_maps.detach(), goal_maps.detach()
        board = ops.StatusBoard.of(dev) if (self.check_solvable and not _capturing(cost_maps)) else None
        row = board.acquire() if board is not None else -1
        cptr = board.counter_ptr(row) if (board is not None and ops.in_lds(H, W)) else 0

        def launch(exact_now: bool, sptr: int, cptr_now: int):
            return ops.search_routes(cost, start, goal, passable, self.g_ratio, max_iters, ops.FLAG_UNIT_COST if unit else 0, route_cap=route_cap,
                                     summary_ptr=sptr, counter_ptr=cptr_now, out_4d=True, exact=exact_now, neighbor_mask=nmask, heuristic=h0,
                                     **({"multi_source": True} if multi else {}))

        try:
            hist, paths, iters, status, _, routes, lengths, costs = launch(exact, board.ptr(row) if board is not None else 0, cptr)
        except BaseException:
            if row >= 0:
                board.release(row)
            raise
        self.last_status, self.last_iters = status, iters
        self._calls += 1
        if row >= 0 and deliver(self._collect_sync(row, dev, bool(cptr)), status, self._calls) and not exact:
            # a finished map of this batch is not at a fixed point of the reference's batch loop (negative costs): the batch again, exactly
            hist, paths, iters, status, _, routes, lengths, costs = launch(True, 0, 0)
            self.last_status, self.last_iters = status, iters
        return RoutedAstarOutput(hist, paths, routes, lengths, costs)

    def cost_to_go(self, cost_maps: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor, policies: bool = True,
                   tiled: bool = False, differentiable: bool = False) -> FieldOutput:
        """The exact cost to the goal from EVERY cell of every map, and the optimal policy that follows it (``ops.cost_to_go``, the kernel of
        include/nastar_fields.h), under this module's own move set: ``neighbor_filter`` through the cached mask.  A move costs the cell being
        left, as the search's g does; ``g_ratio``, ``Tmax`` and the heuristic play no part.  An evaluation call: no autograd graph, detached
        tensors, one host synchronisation for the status.  ``differentiable=True``: ``dists`` carries the gradient to ``cost_maps``
        (include/nastar_fields_grad.h; see ``ops.cost_to_go``): a loss masks the +inf cells itself."""
        return ops.cost_to_go(cost_maps, goal_maps, obstacles_maps, neighbor_mask=self.neighbor_mask(), policies=policies, tiled=tiled,
                              differentiable=differentiable)

    def cost_to_go_tiled(self, cost_maps: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor, policies: bool = True,
                         differentiable: bool = False) -> FieldOutput:
        """``cost_to_go`` by the tiled relaxation (``ops.cost_to_go_tiled``: maps of up to ``ops.FIELDS_TILED_MAX_CELLS`` cells, the same
        bits; the call blocks and cannot be captured), under this module's own move set.  ``differentiable=True``: ``dists`` carries the
        gradient to ``cost_maps`` (include/nastar_fields_grad_tiled.h; its backward blocks too): a loss masks the +inf cells itself."""
        return ops.cost_to_go_tiled(cost_maps, goal_maps, obstacles_maps, neighbor_mask=self.neighbor_mask(), policies=policies,
                                    differentiable=differentiable)[0]

    def soft_cost_to_go(self, cost_maps: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor, tau: float,
                        horizon: Optional[int] = None, policies: bool = False, differentiable: bool = False) -> "ops.SoftFieldOutput":
        """The entropy-regularised (soft-min) cost-to-go field over ``horizon`` moves and, with ``policies``, its soft policy
        (``ops.soft_cost_to_go``, the kernel of include/nastar_soft_fields.h), under this module's own move set.  ``g_ratio``, ``Tmax`` and
        the heuristic play no part.  ``differentiable=True``: ``dists`` carries a gradient to ``cost_maps`` that is smooth in the costs."""
        return ops.soft_cost_to_go(cost_maps, goal_maps, obstacles_maps, tau, horizon, neighbor_mask=self.neighbor_mask(), policies=policies,
                                   differentiable=differentiable)

    def soft_cost_to_go_tiled(self, cost_maps: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor, tau: float,
                              horizon: Optional[int] = None, policies: bool = False, differentiable: bool = False,
                              checkpoint_every: Optional[int] = None) -> "ops.SoftFieldOutput":
        """``soft_cost_to_go`` by tiled sweeps (``ops.soft_cost_to_go_tiled``, the kernels of include/nastar_soft_fields_tiled.h): maps of
        up to 1024x1152, the same bits where both apply.  ``checkpoint_every``: the spacing of the planes the differentiable call keeps
        (None = ceil(sqrt(horizon)); 1 = every plane)."""
        return ops.soft_cost_to_go_tiled(cost_maps, goal_maps, obstacles_maps, tau, horizon, neighbor_mask=self.neighbor_mask(), policies=policies,
                                         differentiable=differentiable, checkpoint_every=checkpoint_every)

    def maxent_path_nll(self, cost_maps: torch.Tensor, start_maps: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor,
                        opt_trajs: torch.Tensor, tau: float, horizon: Optional[int] = None, tiled: bool = False,
                        checkpoint_every: Optional[int] = None) -> torch.Tensor:
        """The negative log-likelihood [B] of the demonstrations ``opt_trajs`` under the maximum-entropy route distribution of
        ``cost_maps`` (``ops.maxent_path_nll``), under this module's own move set.  ``tiled=True``: on the tiled field
        (``ops.maxent_path_nll_tiled``: maps of up to 1024x1152), with its ``checkpoint_every``."""
        if not tiled:
            if checkpoint_every is not None:
                raise ValueError("checkpoint_every belongs to tiled=True: the one-workgroup field keeps every plane")
            return ops.maxent_path_nll(cost_maps, start_maps, goal_maps, obstacles_maps, opt_trajs, tau, horizon, neighbor_mask=self.neighbor_mask())
        return ops.maxent_path_nll_tiled(cost_maps, start_maps, goal_maps, obstacles_maps, opt_trajs, tau, horizon,
                                         neighbor_mask=self.neighbor_mask(), checkpoint_every=checkpoint_every)

    def soft_policy(self, cost_maps: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor, tau: float,
                    horizon: Optional[int] = None) -> "ops.SoftPolicyOutput":
        """The soft field together with the LOG of its soft policy, both differentiable with respect to ``cost_maps``
        (``ops.soft_policy``, the kernels of include/nastar_soft_policy.h), under this module's own move set."""
        return ops.soft_policy(cost_maps, goal_maps, obstacles_maps, tau, horizon, neighbor_mask=self.neighbor_mask())

    def soft_policy_tiled(self, cost_maps: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor, tau: float,
                          horizon: Optional[int] = None, checkpoint_every: Optional[int] = None) -> "ops.SoftPolicyOutput":
        """``soft_policy`` by tiled sweeps (``ops.soft_policy_tiled``, the kernels of include/nastar_soft_policy_tiled.h): maps of up to
        1024x1152, the same bits where both apply.  ``checkpoint_every``: the spacing of the planes a differentiable call keeps (None =
        ceil(sqrt(horizon)); 1 = every plane)."""
        return ops.soft_policy_tiled(cost_maps, goal_maps, obstacles_maps, tau, horizon, neighbor_mask=self.neighbor_mask(),
                                     checkpoint_every=checkpoint_every)

    def policy_nll(self, cost_maps: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor, opt_policies: torch.Tensor,
                   tau: float, horizon: Optional[int] = None, tiled: bool = False, checkpoint_every: Optional[int] = None) -> torch.Tensor:
        """The per-cell imitation loss [B] of the soft policy of ``cost_maps`` against the demonstrated actions ``opt_policies``
        [B,8,H,W] (``ops.soft_policy_nll``), under this module's own move set.  ``tiled=True``: on the tiled policy
        (``ops.soft_policy_nll_tiled``: maps of up to 1024x1152), with its ``checkpoint_every``."""
        if not tiled:
            if checkpoint_every is not None:
                raise ValueError("checkpoint_every belongs to tiled=True: the one-workgroup field keeps every plane")
            return ops.soft_policy_nll(cost_maps, goal_maps, obstacles_maps, opt_policies, tau, horizon, neighbor_mask=self.neighbor_mask())
        return ops.soft_policy_nll_tiled(cost_maps, goal_maps, obstacles_maps, opt_policies, tau, horizon, neighbor_mask=self.neighbor_mask(),
                                         checkpoint_every=checkpoint_every)

    def plan_many(self, cost_maps: torch.Tensor, starts: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor,
                  max_route_len: Optional[int] = None, paths: bool = False) -> FieldRoutesOutput:
        """The ORDERED optimal route from each of S start cells per map to its nearest goal: ONE cost-to-go field per map
        (``ops.cost_to_go`` without policies; the tiled call above ``ops.FIELDS_MAX_CELLS`` cells), then a chase along its policy forest per
        start (``ops.field_routes``, include/nastar_field_routes.h), under this module's own move set.  No search runs: ``g_ratio``,
        ``Tmax`` and the heuristic play no part, the routes are optimal under the search's cost semantics (a move costs the cell being
        left).  ``starts``: an integer [B,S] tensor of flat cell indices, or a float [B,S,H,W] tensor of start maps.  An EVALUATION call: no
        autograd graph, detached tensors.  A failed query (an obstacle or unreachable start, an index outside the map, a zero-cost
        plateau on the way) is reported in ``status``, not raised.  ``max_route_len``: the row length L of ``routes`` (a longer route keeps
        its last L cells); None = the longest route of the call, one more host read.  ``paths=True`` adds the [B,S,H,W] int64 masks of the
        cells in ``routes``."""
        route_cap = _checked_route_len(max_route_len)
        mask = self.neighbor_mask()
        cells = cost_maps.shape[-2] * cost_maps.shape[-1] if torch.is_tensor(cost_maps) and cost_maps.ndim >= 2 else 0
        field = ops.cost_to_go(cost_maps, goal_maps, obstacles_maps, neighbor_mask=mask, policies=False, tiled=cells > ops.FIELDS_MAX_CELLS)
        r = ops.field_routes(field.dists, goal_maps, obstacles_maps, starts, neighbor_mask=mask, max_route_len=route_cap)
        masks = None
        if paths:
            B, S, _ = r.routes.shape
            H, W = field.dists.shape[-2:]
            cell = torch.where(r.routes < 0, H * W, r.routes).long()  # (-1 lands in a spare column)
            masks = torch.zeros((B, S, H * W + 1), dtype=torch.int64, device=cell.device).scatter_(2, cell, 1)[..., :H * W].reshape(B, S, H, W)
        return FieldRoutesOutput(field.dists, r.routes, r.route_lengths, r.route_costs, r.status, masks)

    def sample_routes(self, cost_maps: torch.Tensor, starts: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor, tau: float,
                      num_samples: int = 1, seed: Optional[int] = None, horizon: Optional[int] = None, max_route_len: Optional[int] = None,
                      visits: bool = False) -> "ops.SoftRoutes":
        """``num_samples`` routes from each of S start cells per map, SAMPLED from the maximum-entropy route distribution of ``cost_maps``
        (``ops.soft_routes``, the kernel of include/nastar_soft_routes.h: the soft field with its tape, then one launch of walkers), under
        this module's own move set -- what ``plan_many`` is to the hard field.  ``g_ratio``, ``Tmax`` and the heuristic play no part.  An
        EVALUATION call: no autograd graph, detached tensors, nothing is read back; a failed query is reported in ``status``."""
        return ops.soft_routes(cost_maps, goal_maps, obstacles_maps, starts, tau, horizon, num_samples, seed, neighbor_mask=self.neighbor_mask(),
                               max_route_len=max_route_len, visits=visits)

    def sample_routes_differentiable(self, cost_maps: torch.Tensor, starts: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor,
                                     tau: float, num_samples: int = 1, seed: Optional[int] = None, horizon: Optional[int] = None,
                                     max_route_len: Optional[int] = None, visits: bool = False) -> "ops.SoftRoutes":
        """``sample_routes`` with ``log_probs`` as a differentiable output (``ops.soft_routes(..., differentiable=True)``, include/
        nastar_soft_routes_grad.h): the same launches and the same samples, and a loss on ``log_probs`` -- ``ops.route_score_loss`` with
        any reward per sampled route -- carries the score-function gradient to ``cost_maps``.  Maps of at most
        ``ops.SOFT_ROUTES_GRAD_MAX_CELLS`` cells, rows of ``horizon + 1`` cells (``max_route_len`` None or at least that).  A method of
        its own: ``sample_routes`` keeps its signature."""
        return ops.soft_routes(cost_maps, goal_maps, obstacles_maps, starts, tau, horizon, num_samples, seed, neighbor_mask=self.neighbor_mask(),
                               max_route_len=max_route_len, visits=visits, differentiable=True)

    def sample_routes_tiled(self, cost_maps: torch.Tensor, starts: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor,
                            tau: float, num_samples: int = 1, seed: Optional[int] = None, horizon: Optional[int] = None,
                            max_route_len: Optional[int] = None, visits: bool = False,
                            checkpoint_every: Optional[int] = None) -> "ops.SoftRoutes":
        """``sample_routes`` for maps of up to ``ops.SOFT_FIELDS_TILED_MAX_CELLS`` cells (``ops.soft_routes_tiled``, include/
        nastar_soft_routes_tiled.h: the tiled soft field with its checkpointed tape, then the walkers segment by segment; the same bits on
        the maps both take), under this module's own move set, with the tape's ``checkpoint_every``.  An EVALUATION call; a
        ``max_route_len`` below ``horizon + 1`` rebuilds every segment of the tape twice."""
        return ops.soft_routes_tiled(cost_maps, goal_maps, obstacles_maps, starts, tau, horizon, num_samples, seed,
                                     neighbor_mask=self.neighbor_mask(), max_route_len=max_route_len, visits=visits,
                                     checkpoint_every=checkpoint_every)

    def shortest_paths(self, cost_maps: torch.Tensor, start_maps: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor,
                       lambda_: Optional[float] = None, min_cost: float = 2.0 ** -10) -> PathOutput:
        """The EXACT optimal path of every map as a 0/1 mask (``ops.shortest_paths``, the kernel of include/nastar_path_masks.h: field and
        chase in one launch), under this module's own move set.  No search runs: ``g_ratio``, ``Tmax`` and the heuristic play no part.
        ``lambda_=None``: an evaluation call.  ``lambda_`` a positive float: ``paths`` carries the blackbox gradient to ``cost_maps`` (one
        more launch in the backward, no host read), so that a Hamming or L1 loss on ``paths`` trains whatever produced the costs."""
        return ops.shortest_paths(cost_maps, start_maps, goal_maps, obstacles_maps, neighbor_mask=self.neighbor_mask(), lambda_=lambda_,
                                  min_cost=min_cost)

    def shortest_paths_tiled(self, cost_maps: torch.Tensor, start_maps: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor,
                             lambda_: Optional[float] = None, min_cost: float = 2.0 ** -10) -> PathOutput:
        """``shortest_paths`` for maps of up to ``ops.PATH_MASKS_TILED_MAX_CELLS`` cells (``ops.shortest_paths_tiled``, include/
        nastar_path_masks_tiled.h: the field by the tiled relaxation, the same bits), under this module's own move set.  The call blocks
        and cannot be captured into a graph; with ``lambda_`` the backward of ``paths`` blocks too."""
        return ops.shortest_paths_tiled(cost_maps, start_maps, goal_maps, obstacles_maps, neighbor_mask=self.neighbor_mask(), lambda_=lambda_,
                                        min_cost=min_cost)

    def forward(self, cost_maps: torch.Tensor, start_maps: torch.Tensor, goal_maps: torch.Tensor,
                obstacles_maps: torch.Tensor, store_intermediate_results: bool = False,
                heuristic_maps: Optional[torch.Tensor] = None) -> AstarOutput:
        """``heuristic_maps``: None = the reference's heuristic (today's call, unchanged); a [B,1,H,W] float32 tensor on the device of
        ``cost_maps`` = exactly the reference run with ``astar.get_heuristic = lambda goal_maps: heuristic_maps[:, 0]`` -- zero (Dijkstra),
        weighted, Manhattan, a network's output (any finite values; a NaN / infinite one raises ``ValueError`` naming the map).  A tensor, not
        a callable: a learned heuristic depends on the map, not on the goal alone.  Its gradient is the gradient of ``cost_maps`` (the
        loss sees both only through h = h0 + cost) and flows when either of the two requires one.  With a free heuristic a finished map is
        often not at a fixed point of the reference's batch loop, so a batch of more than one map always runs the exact pipeline (DESIGN.md
        section 2, item 6b).  Composes with ``neighbor_filter``; takes no native host lane, unit-cost layout or hand-scheduled stream.

        ``start_maps`` with SEVERAL non-zero cells in a map: with ``self.multi_source = False`` (the default) the search starts from the one
        with the highest flat index only, silently -- NOT what the reference computes; set ``self.multi_source = True`` for the reference's
        behaviour (every non-zero cell is open with g = 0).  True composes with ``neighbor_filter``,
        ``heuristic_maps``, ``store_intermediate_results``, every ``check_solvable`` mode, autograd and training budgets; it takes no placement,
        native host lane, unit-cost layout, hand-scheduled stream or torch.compile trace, and a one-hot batch gives bit-identical outputs."""
        assert cost_maps.ndim == start_maps.ndim == goal_maps.ndim == obstacles_maps.ndim == 4
        self._refuse_replaced_heuristic()
        h0 = _checked_heuristic(heuristic_maps, cost_maps) if heuristic_maps is not None else None
        self.last_packed = None
        nmask = self.neighbor_mask()  # None: the default (Moore-8) filter -- its kernels, its native host lane, its unit-cost layout
        multi = bool(self.multi_source)
        if multi and torch.compiler.is_compiling():
            raise NotImplementedError("DifferentiableAstar.multi_source = True takes no torch.compile trace (its search is an autograd node of its own, "
                                      "not one of the traceable custom ops): call it outside the compiled region")
        if (not multi and nmask is None and h0 is None and self.check_solvable is True and not store_intermediate_results and not self._pending and type(cost_maps) is torch.Tensor
                and not (cost_maps.requires_grad and torch.is_grad_enabled())):
            out = self._forward_fast(cost_maps, start_maps, goal_maps, obstacles_maps)
            if out is not None:
                return out

        B, _, H, W = cost_maps.shape
        max_iters = ops.max_iters_for(W, self.Tmax, self.training)
        needs_grad = (cost_maps.requires_grad or (h0 is not None and h0.requires_grad)) and torch.is_grad_enabled()
        # the selection log doubles as the tape of the backward (replayed by nastar_backward_replay): keep it whenever
        # autograd will need it
        want_log = bool(store_intermediate_results) or needs_grad
        capturing = cost_maps.is_cuda and torch.cuda.is_current_stream_capturing()
        if self._pending and not capturing:
            self.raise_if_unsolvable(wait=False)  # deferred verdicts of earlier calls that have reached the host
        same = _same_tensor(cost_maps, obstacles_maps)
        mode = self.check_solvable
        # the unit-cost layout pays with SEVERAL launches in flight (more maps resident per CU); one launch at a time is a serial chain whose
        # length does not depend on the layout (probe_boundary: 117 us unit vs 114 us general per placed 4096-map launch), so forward()
        # takes it only on request -- parallel.InFlightPlanner is where "auto" means "unit-cost first"
        unit = same and not want_log and self.unit_cost is True and nmask is None and h0 is None and not multi
        in_lds = ops.in_lds(H, W)
        # a recurring batch starts its longest searches first (Placement), a fresh one by its loader's hint; maps whose state lives in HBM take no placement
        if multi or (self.placement is None and not hasattr(start_maps, "placement_order")):
            order = order_out = pl = None  # (a multi-source call runs in natural order; a pending ``placement`` stays for the next call)
            check_order = False
        else:
            order, order_out, check_order, pl = self.resolve_placement(B, start_maps, in_lds)
            if (nmask is not None or h0 is not None) and needs_grad:
                order = order_out = None  # (a neighbor_filter / a heuristic under autograd: the plain differentiable op, no placement)
        dev = cost_maps.device
        compiling = torch.compiler.is_compiling()
        # (no status protocol while a hipGraph is captured or torch.compile traces: its host side would run once, at capture / trace time)
        board = ops.StatusBoard.of(dev) if (mode and cost_maps.is_cuda and not capturing and not compiling) else None
        row = board.acquire() if board is not None else -1
        sptr = board.ptr(row) if board is not None else 0
        cptr = board.counter_ptr(row) if (board is not None and in_lds) else 0
        flags = ops.FLAG_UNIT_COST if unit else 0
        traced = needs_grad or type(cost_maps) is not torch.Tensor or compiling
        passable_maps = cost_maps if same else obstacles_maps
        exact = needs_exact(B, self.g_ratio, h0 is not None, unit)  # batch semantics: the exact pipeline up front?

        def launch(exact_now: bool, sptr_now: int, cptr_now: int):
            if not traced:
                # no gradient can flow and nothing is tracing: straight to the C ABI (no torch.library dispatch)
                return ops.search_nograd(cost_maps, start_maps, goal_maps, passable_maps, self.g_ratio, max_iters, want_log, flags, order=order,
                                         order_out=order_out, check_order=check_order, summary_ptr=sptr_now, out_4d=True, counter_ptr=cptr_now,
                                         exact=exact_now, neighbor_mask=nmask, heuristic=h0, **({"multi_source": True} if multi else {}))
            cost, start, goal, passable = cost_maps[:, 0], start_maps[:, 0], goal_maps[:, 0], obstacles_maps[:, 0]
            if multi:  # the autograd node of include/nastar_sources.h (the custom ops keep their schemas)
                o = ops.astar_forward_sources(cost, start, goal, passable, self.g_ratio, max_iters, h0[:, 0] if h0 is not None else None, sptr_now,
                                              exact_now, nmask)
                return o[0].unsqueeze(1), o[1].unsqueeze(1), o[2], o[3], o[4]
            mask_arg = ops.NEIGHBORS_MOORE8 if nmask is None else nmask
            heuristic = h0[:, 0] if h0 is not None else None
            placed = order is not None or order_out is not None
            if needs_grad and in_lds and nmask is None and h0 is None and (placed or B >= ops.PLACEMENT_MIN_BATCH):
                # large batches under autograd: the replay backward starts longest-first, by the order THIS forward's searches finish in
                o = ops.astar_forward_placed(cost, start, goal, passable, self.g_ratio, max_iters, flags=0, order_in=order, order_out=order_out,
                                             check_order=check_order, summary_ptr=sptr_now, exact=exact_now)
            elif not placed:
                o = torch.ops.nastar.astar_forward(cost, start, goal, passable, float(self.g_ratio), max_iters, want_log, flags, sptr_now, exact_now,
                                                   mask_arg, heuristic)
            else:
                o = torch.ops.nastar.astar_forward_ordered(cost, start, goal, passable, float(self.g_ratio), max_iters, want_log, flags, order, order_out,
                                                           check_order, sptr_now, exact_now, mask_arg, heuristic)
            return o[0].unsqueeze(1), o[1].unsqueeze(1), o[2], o[3], o[4]

        try:
            hist, paths, iters, status, sel_log = launch(exact, sptr, cptr)
        except BaseException:
            if row >= 0:
                board.release(row)
            raise
        if pl is not None and order_out is not None:
            pl.commit()
        repair = None
        if mode == "deferred" and not exact and B > 1 and row >= 0:
            if needs_grad:
                repair = _refuse_late_repair
            else:  # (no graph holds these tensors: a late verdict that reports the note completes them in place)
                repair = self._repair_in_place((cost_maps, start_maps, goal_maps, passable_maps), (hist, paths, iters, status, sel_log), max_iters, want_log,
                                               nmask, multi)
        if self.note_status(status, iters, row, flagged=bool(cptr) and not traced, repair=repair) and not exact:
            # the same-call verdict says a finished map of this batch is not at a fixed point (negative costs): the batch again, exactly
            order = order_out = None
            hist, paths, iters, status, sel_log = launch(True, 0, 0)
            self.last_status, self.last_iters = status, iters

        intermediate_results: List[dict] = []
        if store_intermediate_results:
            intermediate_results = _intermediate_results(hist[:, 0], paths[:, 0], goal_maps[:, 0], iters, sel_log)
        return AstarOutput(hist, paths, intermediate_results)


def _checked_heuristic(h: torch.Tensor, cost_maps: torch.Tensor) -> torch.Tensor:
    """``heuristic_maps`` of forward(): a [B,1,H,W] float32 tensor on the device of ``cost_maps`` (nothing is launched before this passes)"""
    if not torch.is_tensor(h):
        raise TypeError(f"heuristic_maps must be a tensor of shape [B, 1, H, W] (a callable is not taken: evaluate it first), got {type(h).__name__}")
    if h.dtype != torch.float32:
        raise TypeError(f"heuristic_maps must be float32, got {h.dtype}")
    B, _, H, W = cost_maps.shape
    if h.ndim != 4 or tuple(h.shape) != (B, 1, H, W):
        raise ValueError(f"heuristic_maps must have shape {(B, 1, H, W)} (one value per cell of every map), got {tuple(h.shape)}")
    if h.device != cost_maps.device:
        raise ValueError(f"heuristic_maps lives on {h.device}, cost_maps on {cost_maps.device}: they must share a device")
    if not cost_maps.is_cuda:
        ops._require_device(cost_maps)  # (the package's "no CPU" error)
    return h if h.is_contiguous() else h.contiguous()


def _filter_mask(f) -> int:
    """neighbor_filter -> the 9-bit mask (bit r*3+c <=> cell (r, c) is 1); NotImplementedError, naming the values, for any other filter"""
    if f is None or tuple(f.shape) != (1, 1, 3, 3):
        raise NotImplementedError(f"DifferentiableAstar.neighbor_filter of shape {None if f is None else tuple(f.shape)}: the MI355X search kernels "
                                  "take a [1, 1, 3, 3] filter (the reference's, differentiable_astar.py:140-143)")
    vals = [float(v) for v in f.detach().reshape(-1).cpu().tolist()]
    if any(v not in (0.0, 1.0) for v in vals) or vals[4] != 0.0:
        raise NotImplementedError(f"DifferentiableAstar.neighbor_filter = {vals}: the MI355X search kernels take weights in {{0, 1}} with a zero "
                                  "centre -- any other weight scales g2 and blends the open set and the parent indices in the reference "
                                  "(differentiable_astar.py:228-249), which is not a search; it is refused rather than run as Moore-8")
    return sum(1 << i for i, v in enumerate(vals) if v == 1.0)


_BAD_ORDER_WARNED = False


def _refuse_late_repair() -> None:
    """``check_solvable="deferred"`` under autograd, and the late verdict reports NASTAR_SUMMARY_COUPLED (possible only with NEGATIVE costs when
    g_ratio is in [0.5, 1); every other g_ratio runs the exact pipeline up front): the graph of that call already holds the early-exit
    launch's selection log.  Loud, not silent."""
    raise RuntimeError("a batch searched with check_solvable='deferred' under autograd holds a map that is not at a fixed point of the reference's "
                       "batch loop (negative costs with g_ratio in [0.5, 1)): its histories and gradients depend on the rest of the batch and the call "
                       "that could have completed them has returned.  Use check_solvable=True (the default) for such inputs (DESIGN.md section 2.3)")


def _warn_bad_order() -> None:
    global _BAD_ORDER_WARNED
    if not _BAD_ORDER_WARNED:
        _BAD_ORDER_WARNED = True
        import warnings
        warnings.warn("a placement order handed to the search was not a permutation of 0..B-1: it was ignored (natural order, identical "
                      "outputs); build orders with ops.order_from_levels / Placement", RuntimeWarning, stacklevel=4)  # (past deliver() and the method that read the row)


def _intermediate_results(hist, paths, goal, iters, sel_log) -> List[dict]:
    """Rebuild the reference's per-step side channel (:210-216,:257-263) from the kernel's selection log.

    Entry t holds the histories BEFORE step t and the node selected AT step t; a map that already reached its goal
    keeps re-selecting it (fixed point) until the slowest map of the batch is done; one final entry carries the
    final histories and the int64 path maps."""
    B, H, W = hist.shape
    t_batch = int(iters.max().item()) - 1
    goal_idx = goal.reshape(B, -1).argmax(-1)
    rows = torch.arange(B, device=hist.device)
    cur = torch.zeros((B, H * W), dtype=hist.dtype, device=hist.device)
    out: List[dict] = []
    for t in range(t_batch + 1):
        sel = torch.where(t < iters, sel_log[:, t].long(), goal_idx)
        onehot = torch.zeros_like(cur)
        onehot[rows, sel] = 1
        out.append({"histories": cur.reshape(B, 1, H, W).clone(), "paths": onehot.reshape(B, 1, H, W)})
        cur[rows, sel] = 1
    out.append({"histories": hist.unsqueeze(1).detach(), "paths": paths.unsqueeze(1).detach()})
    return out
