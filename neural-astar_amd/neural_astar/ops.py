"""PyTorch-ROCm custom ops over the C ABI (``include/nastar.h``).

``torch.ops.nastar.astar_forward`` / ``astar_backward_replay`` hand raw device pointers and torch's current HIP stream to
``libnastar_hip.so``.  PyTorch is plumbing here (allocation, streams, autograd bookkeeping); the search itself is
the hand-written HIP kernel.  There is no CPU path: CPU tensors raise.
"""
from __future__ import annotations

import math
import os
from typing import NamedTuple, Optional, Tuple

import torch

from . import _native
from .status import (CLEAN, PROOF_MAX_G_RATIO, STATUS_BAD_HEURISTIC, STATUS_NOT_UNIT_COST, STATUS_UNSOLVABLE, SUMMARY_BAD_ORDER, SUMMARY_COUPLED, SUMMARY_ERRORS,  # noqa: F401
                     SUMMARY_WORDS, StatusBoard, Summary, coupling_possible, needs_exact, proof_covers)  # (a launch's status lives in status.py; the names stay importable from here)

__all__ = ["astar_forward", "astar_backward_replay", "astar_backward_l1_replay", "l1_loss", "astar_l1_loss", "heuristic", "max_iters_for", "search_nograd", "order_from_levels", "OrderHint", "attach_order", "attach_levels",
           "StatusBoard", "route_forward_calls", "search_routes", "source_forward_calls", "astar_forward_sources", "cost_to_go", "FieldOutput", "cost_to_go_tiled",
           "fields_backward", "FIELD_PLATEAU", "FIELDS_GRAD_MAX_CELLS", "fields_backward_tiled", "FIELDS_GRAD_TILED_MAX_CELLS",
           "field_routes", "FieldRoutes", "FIELD_ROUTES_MAX_CELLS", "FIELD_ROUTES_MAX_QUERIES",
           "shortest_paths", "PathOutput", "path_masks", "path_masks_backward", "PATH_MASKS_MAX_CELLS",
           "shortest_paths_tiled", "path_masks_tiled", "path_masks_tiled_backward", "PATH_MASKS_TILED_MAX_CELLS",
           "soft_cost_to_go", "SoftFieldOutput", "maxent_path_nll", "soft_fields_forward", "soft_fields_backward", "SOFT_FIELDS_MAX_CELLS",
           "SOFT_FIELDS_GRAD_MAX_CELLS", "soft_cost_to_go_tiled", "maxent_path_nll_tiled", "soft_fields_tiled_forward",
           "soft_fields_tiled_backward", "SOFT_FIELDS_TILED_MAX_CELLS",
           "soft_policy", "SoftPolicyOutput", "soft_policy_nll", "soft_policy_forward", "soft_policy_backward",
           "soft_policy_tiled", "soft_policy_nll_tiled", "soft_policy_tiled_forward", "soft_policy_tiled_backward",
           "soft_routes", "SoftRoutes", "soft_routes_from_tape", "SOFT_ROUTES_MAX_CELLS", "SOFT_ROUTES_MAX_WALKERS", "soft_routes_tiled",
           "soft_routes_tiled_from_tape", "soft_routes_backward", "route_score_loss", "SOFT_ROUTES_GRAD_MAX_CELLS"]


def max_iters_for(W: int, Tmax: float, training: bool) -> int:
    """Search budget exactly as the reference computes it (differentiable_astar.py:200-202)."""
    t = Tmax if training else 1.0
    return int(t * W * W)


def _require_device(*tensors: torch.Tensor) -> None:
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError(
                "neural_astar (MI355X-native): tensors must live on a HIP device; this package has no CPU "
                "fallback for the A* search (the reference's CPU path is the oracle under oracle/, test-only).")
        if t.dtype != torch.float32:
            raise TypeError(f"expected float32 maps, got {t.dtype}")


FLAG_UNIT_COST = 64  # include/nastar.h NASTAR_FLAG_UNIT_COST
FLAG_LOCKSTEP = 1024  # NASTAR_FLAG_LOCKSTEP: the reference's batch loop to the letter (no exit at the goal; exactly max_iters steps)
FLAG_CHECK_ORDER = 256  # NASTAR_FLAG_CHECK_ORDER: the launch verifies `order` on the device and ignores it when it is not a permutation
FLAG_MARK_COUPLED = 32768  # NASTAR_FLAG_MARK_COUPLED: the launch marks the maps of the batch-coupled class for nastar_forward_batchloop_finish
# DifferentiableAstar.neighbor_filter as a 9-bit mask (include/nastar.h NASTAR_NEIGHBORS_*): bit r*3+c <=> filter cell (r, c) is 1
NEIGHBORS_MOORE8 = 0x1EF
NEIGHBORS_VON_NEUMANN = 0x0AA
# development knob: flag bits OR-ed into every forward launch.  NASTAR_FLAG_UNIT_COST = 64 works with the product library; the A/B switches
# of csrc/nastar_dev_flags.h (NO_ASM = 8, ASM_V2 = 16, NO_DIVE = 32, ASM_V3 = 128) need the development build: NASTAR_LIB=.../libnastar_hip_dev.so
FORWARD_FLAGS = int(os.environ.get("NASTAR_FORWARD_FLAGS", "0"))
if FORWARD_FLAGS & ~(8 | 16 | 32 | 64 | 128):
    raise ValueError(f"NASTAR_FORWARD_FLAGS={FORWARD_FLAGS}: unknown flag bits (include/nastar.h NASTAR_FLAG_*, csrc/nastar_dev_flags.h)")


def _stream_ptr(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _order_ptr(order: torch.Tensor, B: int, dev: torch.device, buffer_ok: bool = False) -> int:
    """``buffer_ok``: also accept the [B + 1] ``order_out`` buffer of the forward launch as it is (the replay backward reads its first B cells)"""
    if (order.dtype != torch.int32 or (order.numel() != B and not (buffer_ok and order.numel() == B + 1)) or order.device != dev
            or not order.is_contiguous()):
        raise ValueError(f"order must be a contiguous int32 tensor of exactly {B} elements on {dev} (got {tuple(order.shape)} {order.dtype} on {order.device})")
    return order.data_ptr()


# batches from this size on replay their backward longest-first, by the order the forward's searches finished in (one 4 x (B + 1)-byte
# fill per step buys it; 4096 mazes at Tmax 0.25: 187 -> 133 us for the replay; below ~1000 maps every search has a SIMD to itself)
PLACEMENT_MIN_BATCH = 1024


def _maps3(t: torch.Tensor) -> torch.Tensor:
    """[B,1,H,W] or [B,C,H,W] (channel 0 is used, differentiable_astar.py:177-180) -> contiguous [B,H,W]."""
    if t.ndim == 4:
        t = t[:, 0]
    return t.contiguous()


_IN_LDS: dict = {}


def in_lds(H: int, W: int) -> bool:
    """does the search state of an H x W map live in LDS (no HBM workspace; placements apply)?  Cached per size."""
    v = _IN_LDS.get((H, W))
    if v is None:
        v = _IN_LDS[(H, W)] = int(_native.load().nastar_workspace_bytes(1, H, W, 0)) == 0
    return v


def _entry_family(neighbor_mask: Optional[int], heuristic, multi_source: bool = False):
    """THE choice among the three twins of every search / finish / ordered-replay entry point (include/nastar.h): -> (suffix of the symbol,
    the arguments it takes between the base entry's and the stream).  Plain: no mask (None -- Moore-8 on the fastest kernels) and no
    heuristic; `_masked`: a mask, NEIGHBORS_MOORE8 included; `_heuristic`: a heuristic, with the given mask or Moore-8.
    ``multi_source``: the family of include/nastar_sources.h instead (`_sources`: nastar_forward_sources, nastar_forward_sources_batchloop_finish,
    nastar_backward_replay_sources) -- always a mask (Moore-8 by default) and a heuristic slot that may stay empty."""
    if multi_source:
        return "_sources", (NEIGHBORS_MOORE8 if neighbor_mask is None else int(neighbor_mask), heuristic or None)
    if heuristic is not None:
        return "_heuristic", (NEIGHBORS_MOORE8 if neighbor_mask is None else int(neighbor_mask), heuristic)
    if neighbor_mask is not None:
        return "_masked", (int(neighbor_mask),)
    return "", ()


def forward_calls(cost, start, goal, passable, B, H, W, g_ratio, max_iters, histories_out, paths_out, sel_log_out, iters_out, status_out,
                  workspace, workspace_bytes, flags, order, order_out, status_summary, completion_counter, stream, exact=False,
                  neighbor_mask=None, h0=None):
    """The C calls of ONE search as plain values (addresses as ints, None / 0 = absent; no tensor, no device): -> ((symbol, arguments) of the
    launch, (symbol, arguments) of the batch-loop finish behind it -- None unless ``exact``).  The parameters up to ``stream`` ARE those of
    nastar_forward_ex in include/nastar.h, names and order (less packed_out; tests/test_capi_library.py pins it): ``_launch_search`` passes
    them by position -- keywords cost the Python lane 1.5 us per launch.  ``completion_counter`` goes out only with a ``status_summary``."""
    suffix, tail = _entry_family(neighbor_mask, h0)
    problem = (cost, start, goal, passable, B, H, W, float(g_ratio), int(max_iters), histories_out, paths_out, sel_log_out or None, iters_out,
               status_out)
    launch = ("nastar_forward_ex" + suffix,
              (*problem, None, workspace or None, workspace_bytes, flags, order or None, order_out or None, status_summary or None,
               (completion_counter or None) if status_summary else None, *tail, stream))
    finish = ("nastar_forward_batchloop_finish" + suffix, (*problem, workspace, workspace_bytes, *tail, stream)) if exact else None
    return launch, finish


def _routed_calls(multi_source, cost, start, goal, passable, B, H, W, g_ratio, max_iters, histories_out, paths_out, sel_log_out, iters_out, status_out,
                  workspace, workspace_bytes, flags, order, order_out, status_summary, completion_counter, neighbor_mask, h0, routes_out, route_cap,
                  route_len_out, route_cost_out, stream, exact):
    """the one assembler behind ``route_forward_calls`` and ``source_forward_calls``: both headers give their launch the parameters of
    nastar_forward_routes and their finish those of nastar_forward_routes_batchloop_finish; the family (``_entry_family``) names the symbols"""
    problem = (cost, start, goal, passable, B, H, W, float(g_ratio), int(max_iters), histories_out, paths_out, sel_log_out or None, iters_out,
               status_out)
    if multi_source:
        suffix, family = _entry_family(neighbor_mask, h0, True)
        names = ("nastar_forward" + suffix, "nastar_forward" + suffix + "_batchloop_finish")
        routes = (routes_out, int(route_cap), route_len_out, route_cost_out or None) if routes_out else (None, 0, None, None)  # optional here
    else:
        family = (NEIGHBORS_MOORE8 if neighbor_mask is None else int(neighbor_mask), h0 or None)
        names = ("nastar_forward_routes", "nastar_forward_routes_batchloop_finish")
        routes = (routes_out, int(route_cap), route_len_out, route_cost_out or None)
    tail = (*family, *routes, stream)
    launch = (names[0], (*problem, None, workspace or None, workspace_bytes, flags, order or None, order_out or None, status_summary or None,
                         (completion_counter or None) if status_summary else None, *tail))
    finish = (names[1], (*problem, workspace, workspace_bytes, *tail)) if exact else None
    return launch, finish


def route_forward_calls(cost, start, goal, passable, B, H, W, g_ratio, max_iters, histories_out, paths_out, sel_log_out, iters_out, status_out,
                        workspace, workspace_bytes, flags, order, order_out, status_summary, completion_counter, neighbor_mask, h0, routes_out,
                        route_cap, route_len_out, route_cost_out, stream, exact=False):
    """``forward_calls`` for the launch that also returns ordered routes (include/nastar_routes.h): -> ((nastar_forward_routes, arguments),
    (nastar_forward_routes_batchloop_finish, arguments) -- None unless ``exact``).  The parameters up to ``stream`` ARE those of
    nastar_forward_routes, names and order (less packed_out; tests/test_routes.py pins it).  ONE entry point serves every neighbourhood:
    ``neighbor_mask`` None = Moore-8, ``h0`` None = the reference's heuristic -- both None is the launch of nastar_forward_ex."""
    return _routed_calls(False, cost, start, goal, passable, B, H, W, g_ratio, max_iters, histories_out, paths_out, sel_log_out, iters_out, status_out,
                         workspace, workspace_bytes, flags, order, order_out, status_summary, completion_counter, neighbor_mask, h0, routes_out,
                         route_cap, route_len_out, route_cost_out, stream, exact)


def source_forward_calls(cost, start, goal, passable, B, H, W, g_ratio, max_iters, histories_out, paths_out, sel_log_out, iters_out, status_out,
                         workspace, workspace_bytes, flags, order, order_out, status_summary, completion_counter, neighbor_mask, h0, routes_out,
                         route_cap, route_len_out, route_cost_out, stream, exact=False):
    """``route_forward_calls`` for the MULTI-SOURCE launch (include/nastar_sources.h: every non-zero cell of the start maps is a source): ->
    ((nastar_forward_sources, arguments), (nastar_forward_sources_batchloop_finish, arguments) -- None unless ``exact``).  The parameters up
    to ``stream`` ARE those of nastar_forward_sources, names and order (less packed_out; tests/test_multisource.py pins it).  The route outputs
    are optional here: ``routes_out`` None = no routes (the other three then go out as NULL / 0 too)."""
    return _routed_calls(True, cost, start, goal, passable, B, H, W, g_ratio, max_iters, histories_out, paths_out, sel_log_out, iters_out, status_out,
                         workspace, workspace_bytes, flags, order, order_out, status_summary, completion_counter, neighbor_mask, h0, routes_out,
                         route_cap, route_len_out, route_cost_out, stream, exact)


def replay_call(*, cost, start, goal, passable, sel_log, B, H, W, g_ratio, max_iters, iters, t_batch, grad_cost, workspace, ws_bytes, stream,
                grad_hist=None, histories=None, opt_trajs=None, grad_loss=None, flags=0, order=None, neighbor_mask=None, heuristic=None,
                multi_source=False):
    """The C call of ONE replay backward as plain values: -> (symbol, arguments).  ``grad_hist`` given: dL/dhistories comes from autograd;
    None: the fused L1 form (``histories``, ``opt_trajs``, ``grad_loss``).  nastar_backward_replay / nastar_backward_l1_replay where they
    suffice (no order, mask or heuristic; the L1 one takes no flags either), the `_ordered` family otherwise.  ``multi_source``: the log of a
    multi-source search -- nastar_backward_replay_sources (include/nastar_sources.h), one entry point for every mask, heuristic and order."""
    suffix, tail = _entry_family(neighbor_mask, heuristic, multi_source)
    replay = (cost, start, goal, passable, sel_log, B, H, W, float(g_ratio), int(max_iters), iters, t_batch, grad_cost, workspace, ws_bytes)
    if multi_source:
        return "nastar_backward_replay" + suffix, (grad_hist, histories, opt_trajs, grad_loss) + replay + (int(flags), order) + tail + (stream,)
    if not suffix and order is None:
        if grad_hist is not None:
            return "nastar_backward_replay", (grad_hist,) + replay + (int(flags), stream)
        if not flags:
            return "nastar_backward_l1_replay", (histories, opt_trajs, grad_loss) + replay + (stream,)
    return "nastar_backward_replay_ordered" + suffix, (grad_hist, histories, opt_trajs, grad_loss) + replay + (int(flags), order) + tail + (stream,)


def _launch_search(lib, cost, start, goal, passable, B, H, W, g_ratio, max_iters, want_log, flags, dev, order=None, order_out=None,
                   check_order=False, summary_ptr=0, one_meta=False, stream_ptr=None, out_4d=False, counter_ptr=0, keep=None, exact=False,
                   neighbor_mask=None, heuristic=None, route_cap=None, multi_source=False):
    """allocate the five outputs and issue ONE nastar_forward_ex launch on torch's current stream (shared by the custom ops and the
    no-autograd fast path).  cost / start / goal / passable: contiguous fp32 tensors of B*H*W elements (any leading shape).
    ``keep``: a list that receives the launch's temporaries (its workspace) when the launch goes to ANOTHER stream than the one the
    caching allocator hands the memory out for -- the caller holds them until that stream is done.
    ``exact``: the reference's BATCH LOOP to the letter (include/nastar.h: nastar_forward_batchloop_finish) -- the launch marks the maps that
    are not at a fixed point of that loop when they reach their goal, and three more launches on the same stream re-run exactly those in
    lock-step mode up to the step at which every map of the batch selects its goal.  No host round trip; nothing happens when no map is
    marked (always so for g_ratio in [0.5, 1) with costs >= 0).
    ``neighbor_mask``: None = the reference's default neighbourhood (Moore-8) on the fastest kernels; an int = the search neighbourhood of a
    ``neighbor_filter`` (NEIGHBORS_*), searched by the masked entry points (nastar_forward_ex_masked: the compiled step loops, for every mask).
    ``heuristic``: None = the reference's get_heuristic, computed by the kernels; a contiguous fp32 [B, H, W] tensor = the caller's heuristic
    maps (nastar_forward_ex_heuristic; with ``neighbor_mask`` or Moore-8).  Which symbols are called with which arguments: ``forward_calls``.
    ``route_cap``: None = the five outputs; an int >= 1 = the launch of include/nastar_routes.h (``route_forward_calls``: same kernels, same
    five outputs) that also writes routes [B, route_cap] int32, route lengths [B] int32 and route costs [B] float32 -- three more results.
    ``multi_source``: the launch of include/nastar_sources.h (``source_forward_calls``) -- every non-zero cell of ``start`` is a source; with or
    without ``route_cap``."""
    shape = (B, 1, H, W) if out_4d else (B, H, W)
    hist = torch.empty(shape, dtype=torch.float32, device=dev)
    paths = torch.empty(shape, dtype=torch.int64, device=dev)
    if one_meta:  # iters, status: one allocation (not for the custom ops, whose outputs must not alias each other)
        meta = torch.empty((2, B), dtype=torch.int32, device=dev)
        iters, status = meta[0], meta[1]
    else:
        iters = torch.empty((B,), dtype=torch.int32, device=dev)
        status = torch.empty((B,), dtype=torch.int32, device=dev)
    # entries at positions >= iters[b] are never read (the backward replays iters[b] steps, _intermediate_results masks by iters)
    sel_log = torch.empty((B, max_iters), dtype=torch.int32, device=dev) if want_log else (None if out_4d else torch.empty((0,), dtype=torch.int32, device=dev))
    flags = int(flags) | FORWARD_FLAGS
    order_ptr = None
    if order is not None:
        order_ptr = _order_ptr(order, B, dev)
        if check_order:
            flags |= FLAG_CHECK_ORDER
    if order_out is not None and (order_out.dtype != torch.int32 or order_out.numel() != B + 1 or order_out.device != dev or not order_out.is_contiguous()):
        raise ValueError(f"order_out must be a contiguous int32 tensor of exactly {B + 1} elements on {dev} (ops.new_placement_buffer)")
    # workspace: > 0 for maps too large for LDS, for a checked order and for the marks / probe bitmaps of an exact launch
    if exact and B > 1 and not (flags & FLAG_LOCKSTEP):
        flags |= FLAG_MARK_COUPLED
        ws_bytes = int(lib.nastar_batchloop_workspace_bytes(B, H, W, int(max_iters)))
    else:
        exact = False  # (a map on its own is its own batch: the loop ends at its goal step)
        ws_bytes = (16 if flags & FLAG_CHECK_ORDER else 0) if in_lds(H, W) else int(lib.nastar_workspace_bytes(B, H, W, flags))
    workspace = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev) if ws_bytes else None
    if stream_ptr is not None and workspace is not None:
        if keep is None:
            raise ValueError("a launch on a foreign stream that needs a workspace must be given a `keep` list (the allocator would hand the "
                             "workspace to the next launch on the current stream while this one still runs)")
        keep.append(workspace)
    stream = stream_ptr if stream_ptr is not None else torch.cuda.current_stream(dev).cuda_stream
    fixed = (cost.data_ptr(), start.data_ptr(), goal.data_ptr(), passable.data_ptr(), B, H, W, g_ratio, max_iters, hist.data_ptr(), paths.data_ptr(),
             sel_log.data_ptr() if want_log else None, iters.data_ptr(), status.data_ptr(), workspace.data_ptr() if workspace is not None else None,
             ws_bytes, flags, order_ptr, order_out.data_ptr() if order_out is not None else None, summary_ptr, counter_ptr)
    h0_ptr = heuristic.data_ptr() if heuristic is not None else None
    if route_cap is None and not multi_source:
        (fwd, args), fin = forward_calls(*fixed, stream, exact, neighbor_mask, h0_ptr)
    else:  # the routed families: include/nastar_routes.h, include/nastar_sources.h (its routes are optional)
        routes = route_len = route_cost = None
        if route_cap is not None:
            routes = torch.empty((B, route_cap), dtype=torch.int32, device=dev)
            route_len = torch.empty((B,), dtype=torch.int32, device=dev)
            route_cost = torch.empty((B,), dtype=torch.float32, device=dev)
        (fwd, args), fin = _routed_calls(bool(multi_source), *fixed, neighbor_mask, h0_ptr, routes.data_ptr() if routes is not None else None,
                                         route_cap or 0, route_len.data_ptr() if routes is not None else None,
                                         route_cost.data_ptr() if routes is not None else None, stream, exact)
    if dev.index is None or torch.cuda.current_device() == dev.index:
        rc = getattr(lib, fwd)(*args)
        if not rc and fin is not None:
            rc = getattr(lib, fin[0])(*fin[1])
    else:
        with torch.cuda.device(dev):
            rc = getattr(lib, fwd)(*args)
            if not rc and fin is not None:
                rc = getattr(lib, fin[0])(*fin[1])
    if rc:
        _native.check(rc, fwd)
    if route_cap is not None:
        return hist, paths, iters, status, sel_log, routes, route_len, route_cost
    return hist, paths, iters, status, sel_log


@torch.library.custom_op("nastar::astar_forward", mutates_args=())
def astar_forward(cost: torch.Tensor, start: torch.Tensor, goal: torch.Tensor, passable: torch.Tensor,
                  g_ratio: float, max_iters: int, want_log: bool, flags: int = 0, summary_ptr: int = 0, exact: bool = False,
                  neighbor_mask: int = NEIGHBORS_MOORE8,
                  heuristic: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Returns (histories [B,H,W] f32, paths [B,H,W] i64, iters [B] i32, status [B] i32, sel_log [B,T] i32 or [0]).
    ``flags``: NASTAR_FLAG_* of include/nastar.h (e.g. ``FLAG_UNIT_COST`` when cost and passable are ONE binary tensor);
    ``summary_ptr``: address of a ``StatusBoard`` row (0 = none) that receives the launch's status summary; ``exact``: see ``_launch_search``;
    ``neighbor_mask``: the search neighbourhood (NEIGHBORS_*, DifferentiableAstar.neighbor_filter); the backward replays with the same one.
    ``heuristic``: [B,H,W] fp32 heuristic maps in place of the reference's get_heuristic (None = that one); its gradient is the cost's."""
    return _op_search(cost, start, goal, passable, g_ratio, max_iters, want_log, flags, neighbor_mask, heuristic, summary_ptr=summary_ptr, exact=exact)


def _op_search(cost, start, goal, passable, g_ratio, max_iters, want_log, flags, neighbor_mask, heuristic, **options):
    """body of the two forward ops: [B,H,W] tensors as they come -> ``_launch_search``"""
    _require_device(cost, start, goal, passable)
    lib = _native.load()
    cost, start, goal, passable = (x.contiguous() for x in (cost, start, goal, passable))
    B, H, W = cost.shape
    return _launch_search(lib, cost, start, goal, passable, B, H, W, g_ratio, max_iters, want_log, flags, cost.device,
                          neighbor_mask=_mask_arg(neighbor_mask), heuristic=_heuristic_arg(heuristic, cost), **options)


def _op_search_fake(cost, max_iters, want_log):
    B, H, W = cost.shape
    return (cost.new_empty((B, H, W)), cost.new_empty((B, H, W), dtype=torch.int64),
            cost.new_empty((B,), dtype=torch.int32), cost.new_empty((B,), dtype=torch.int32),
            cost.new_empty((B, max_iters) if want_log else (0,), dtype=torch.int32))


def _mask_arg(neighbor_mask: int) -> Optional[int]:
    """the custom ops' `neighbor_mask` -> ``_entry_family``'s: Moore-8 keeps the entry points (and kernels) without a mask"""
    return None if int(neighbor_mask) == NEIGHBORS_MOORE8 else int(neighbor_mask)


def _heuristic_arg(heuristic: Optional[torch.Tensor], cost: torch.Tensor) -> Optional[torch.Tensor]:
    """the custom ops' `heuristic` -> ``_launch_search``'s: contiguous fp32 [B,H,W] on the device of ``cost``"""
    if heuristic is None:
        return None
    _require_device(heuristic)
    if heuristic.shape != cost.shape or heuristic.device != cost.device:
        raise ValueError(f"heuristic must have the shape and device of cost ({tuple(cost.shape)} on {cost.device}), got {tuple(heuristic.shape)} on {heuristic.device}")
    return heuristic.contiguous()


@astar_forward.register_fake
def _(cost, start, goal, passable, g_ratio, max_iters, want_log, flags=0, summary_ptr=0, exact=False, neighbor_mask=NEIGHBORS_MOORE8, heuristic=None):
    return _op_search_fake(cost, max_iters, want_log)


@torch.library.custom_op("nastar::astar_forward_ordered", mutates_args=("order_out",))
def astar_forward_ordered(cost: torch.Tensor, start: torch.Tensor, goal: torch.Tensor, passable: torch.Tensor, g_ratio: float,
                          max_iters: int, want_log: bool, flags: int, order: Optional[torch.Tensor],
                          order_out: Optional[torch.Tensor], check_order: bool = True, summary_ptr: int = 0, exact: bool = False,
                          neighbor_mask: int = NEIGHBORS_MOORE8,
                          heuristic: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """``astar_forward`` with a placement (include/nastar.h: nastar_forward_ex): workgroup i searches map ``order[i]`` (int32 [B], a
    permutation of 0..B-1, or None = identity).  Same five outputs as ``astar_forward``.  ``order_out`` (int32 [B + 1] from
    ``new_placement_buffer``, or None) receives in [:B] the maps in reverse order of search completion in this launch -- the ``order``
    for the next visit of the same batch; its last cell is the launch's counter (0 before and after).  ``check_order`` (default): the
    launch verifies ``order`` on the device (one small launch) and searches in the natural order when it is not a permutation -- every
    map is searched whatever the caller passed; False only for orders that are permutations by construction (an earlier launch's
    ``order_out``, ``order_from_levels``, ``placement_predict``, an argsort).  No autograd."""
    return _op_search(cost, start, goal, passable, g_ratio, max_iters, want_log, flags, neighbor_mask, heuristic, order=order, order_out=order_out,
                      check_order=check_order, summary_ptr=summary_ptr, exact=exact)


@astar_forward_ordered.register_fake
def _(cost, start, goal, passable, g_ratio, max_iters, want_log, flags, order, order_out, check_order=True, summary_ptr=0, exact=False,
      neighbor_mask=NEIGHBORS_MOORE8, heuristic=None):
    return _op_search_fake(cost, max_iters, want_log)


def search_nograd(cost_maps: torch.Tensor, start_maps: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor, g_ratio: float,
                  max_iters: int, want_log: bool = False, flags: int = 0, *, order: Optional[torch.Tensor] = None,
                  order_out: Optional[torch.Tensor] = None, check_order: bool = True, summary_ptr: int = 0, stream_ptr: Optional[int] = None,
                  out_4d: bool = False, counter_ptr: int = 0, keep: Optional[list] = None, exact: bool = False, lib=None,
                  neighbor_mask: Optional[int] = None, heuristic: Optional[torch.Tensor] = None, route_cap: Optional[int] = None,
                  multi_source: bool = False):
    """The search launch WITHOUT the torch.library dispatch: what ``DifferentiableAstar.forward`` calls when no gradient can flow
    (``torch.no_grad()`` / inputs that do not require one) and nothing is being traced -- the custom-op machinery costs more host time
    than the launch itself at 4096 maps.  Takes the reference's [B,1,H,W] tensors (or [B,H,W]) as they are; same five outputs
    (``out_4d``: histories / paths as [B,1,H,W], the AstarOutput layout, and None instead of an empty selection log).
    ``summary_ptr`` / ``counter_ptr``: a ``StatusBoard`` row (status summary in pinned memory + its completion counter on the device).
    ``stream_ptr``: a hipStream_t to launch on instead of torch's current stream (``parallel.InFlightPlanner``; the outputs are
    allocated on the CURRENT stream: the caller orders the two streams before anyone reads or frees them, passes contiguous inputs --
    a copy made here would be made on the current stream, after the caller ordered the streams -- and holds ``keep``, the list that
    receives the launch's workspace, until that stream is done).  ``exact``: the reference's batch loop to the letter (``_launch_search``).
    ``lib``: another build of the C ABI (``_native.load_dev()``: stream-equality tests).  ``neighbor_mask``, ``heuristic`` ([B,1,H,W] or
    [B,H,W] fp32 on the maps' device; made contiguous here): see ``_launch_search``.  ``route_cap``: what ``search_routes`` passes.
    ``multi_source``: every non-zero cell of ``start_maps`` is a source (include/nastar_sources.h); False = the highest-index one only."""
    if stream_ptr is not None and not (cost_maps.is_contiguous() and start_maps.is_contiguous() and goal_maps.is_contiguous()
                                       and obstacles_maps.is_contiguous()):
        raise ValueError("search_nograd(stream_ptr=...): the maps must be contiguous (make the copies before ordering the streams)")
    if not (cost_maps.is_cuda and start_maps.is_cuda and goal_maps.is_cuda and obstacles_maps.is_cuda
            and cost_maps.dtype == start_maps.dtype == goal_maps.dtype == obstacles_maps.dtype == torch.float32):
        _require_device(cost_maps, start_maps, goal_maps, obstacles_maps)
    same = obstacles_maps is cost_maps
    if cost_maps.ndim == 4 and not (cost_maps.shape[1] == start_maps.shape[1] == goal_maps.shape[1] == obstacles_maps.shape[1] == 1):
        cost_maps, start_maps, goal_maps, obstacles_maps = (x[:, 0] for x in (cost_maps, start_maps, goal_maps, obstacles_maps))
    B, H, W = cost_maps.shape[0], cost_maps.shape[-2], cost_maps.shape[-1]
    n = B * H * W
    if not (start_maps.numel() == n and goal_maps.numel() == n and obstacles_maps.numel() == n
            and start_maps.shape[-2:] == cost_maps.shape[-2:] == goal_maps.shape[-2:] == obstacles_maps.shape[-2:]):
        raise ValueError("cost / start / goal / obstacle maps must have one shape")
    if not cost_maps.is_contiguous():
        cost_maps = cost_maps.contiguous()
    if same:
        obstacles_maps = cost_maps
    elif not obstacles_maps.is_contiguous():
        obstacles_maps = obstacles_maps.contiguous()
    if not start_maps.is_contiguous():
        start_maps = start_maps.contiguous()
    if not goal_maps.is_contiguous():
        goal_maps = goal_maps.contiguous()
    if heuristic is not None:
        if not (heuristic.is_cuda and heuristic.dtype == torch.float32):
            _require_device(heuristic)
        if heuristic.numel() != n or heuristic.shape[-2:] != cost_maps.shape[-2:] or heuristic.device != cost_maps.device:
            raise ValueError("heuristic maps must have the shape and device of the cost maps")
        if not heuristic.is_contiguous():
            heuristic = heuristic.contiguous()
    # (the options by position, in ``_launch_search``'s order, here alone: twelve keywords cost this lane 1 us per launch -- the ops pass keywords;
    # the True is one_meta)
    return _launch_search(lib if lib is not None else _native.load(), cost_maps, start_maps, goal_maps, obstacles_maps, B, H, W, g_ratio, max_iters,
                          want_log, flags, cost_maps.device, order, order_out, check_order, summary_ptr, True, stream_ptr, out_4d, counter_ptr,
                          keep, exact, neighbor_mask, heuristic, route_cap, multi_source)


def search_routes(cost_maps: torch.Tensor, start_maps: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor, g_ratio: float,
                  max_iters: int, flags: int = 0, *, route_cap: Optional[int] = None, **options):
    """The search launch that also returns every map's ORDERED route (include/nastar_routes.h): a no-grad call to the C ABI, same kernels and
    same first five outputs as ``search_nograd`` (whose ``options`` it takes: order, order_out, check_order, summary_ptr, counter_ptr, out_4d,
    exact, neighbor_mask, heuristic) -> (histories, paths, iters, status, sel_log, routes [B, route_cap] int32, route_lengths [B] int32,
    route_costs [B] float32).  Row b of ``routes``: the last min(len, route_cap) cells of the route as flat indices r*W + c, the goal last
    among them, then -1; ``route_lengths`` is the true length whatever the capacity; ``route_costs`` the fp64 sum of the costs of the route
    cells but the goal, rounded once.  ``route_cap``: None = min(H*W, max_iters + 1), which always suffices."""
    H, W = int(cost_maps.shape[-2]), int(cost_maps.shape[-1])
    if route_cap is None:
        route_cap = min(H * W, int(max_iters) + 1)
    if isinstance(route_cap, bool) or not isinstance(route_cap, int) or route_cap < 1:
        raise ValueError(f"route_cap must be an int >= 1, got {route_cap!r}")
    return search_nograd(cost_maps, start_maps, goal_maps, obstacles_maps, g_ratio, max_iters, False, flags, route_cap=route_cap, **options)


def order_from_levels(levels: torch.Tensor) -> torch.Tensor:
    """``order`` ([B] int32) for ``astar_forward_ordered`` from data the caller already HAS: ``levels[b]`` = any non-negative number that
    grows with the expected length of map b's search -- for the reference's maze data sets the optimal distance of the sampled start
    cell, ``|opt_dists[start]|``, which every sample carries (reference utils/data.py:127-134, :200-221).  Largest first; one
    counting-sort launch (include/nastar.h: nastar_placement_from_levels).  A permutation by construction (``check_order=False``)."""
    if not levels.is_cuda:
        raise RuntimeError("order_from_levels: levels must live on a HIP device")
    lv = levels.reshape(-1).abs().to(torch.int32).contiguous() if levels.dtype != torch.int32 else levels.reshape(-1).contiguous()
    B = lv.numel()
    order = torch.empty((B,), dtype=torch.int32, device=lv.device)
    with torch.cuda.device(lv.device):
        rc = _native.load().nastar_placement_from_levels(lv.data_ptr(), B, order.data_ptr(), _stream_ptr(lv.device))
    _native.check(rc, "nastar_placement_from_levels")
    return order


class OrderHint:
    """A placement for ONE batch, attached to its ``start_maps`` tensor as ``start_maps.placement_order`` by whoever assembled the batch
    (``DeviceMazeBatches``, ``order_hint_from_distances``): the reference's 4-tuple batches keep their shape, ``PlannerModule`` and
    ``DifferentiableAstar.forward`` pick the hint up from the tensor.  ``trusted`` = a permutation by construction."""

    __slots__ = ("order", "trusted", "levels")

    def __init__(self, order: Optional[torch.Tensor], trusted: bool = False, levels: Optional[torch.Tensor] = None):
        self.order, self.trusted, self.levels = order, trusted, levels

    def resolve(self) -> Optional[torch.Tensor]:
        """the order, computed from the levels on first use (``attach_levels``)"""
        if self.order is None and self.levels is not None:
            self.order, self.trusted = order_from_levels(self.levels), True
        return self.order


def attach_order(start_maps: torch.Tensor, levels: torch.Tensor) -> torch.Tensor:
    """tag ``start_maps`` with the placement ``order_from_levels(levels)`` (the sort runs NOW: batch assembly); returns ``start_maps``"""
    start_maps.placement_order = OrderHint(order_from_levels(levels), trusted=True)
    return start_maps


def attach_levels(start_maps: torch.Tensor, levels: torch.Tensor) -> torch.Tensor:
    """tag ``start_maps`` with the LEVELS its loader has (``levels[b]`` = |opt_dists[start]| of map b, int32 [B] on the device; see
    ``order_from_levels``) and leave the placement to the ``forward()`` call that searches the batch.  For 16x16, 32x32 and 64x64 maps on the
    hand-scheduled streams the search launch places the maps itself (include/nastar_levels.h): with ``nblk = ceil(B / 64)``, workgroup ``i``
    looks at the at most 64 maps ``j, j + nblk, j + 2 nblk, ...`` (``j = i % nblk``) and searches the one with exactly ``i // nblk`` of them
    ahead of it, larger level first, lower index first among equals -- a permutation whatever the levels hold, the longest map of every
    block in the first ``nblk`` workgroups, and no sort launch.  Every other launch (unit-cost layout, compiled loops) sorts: its counting-sort
    launch goes out right in front of the search launch, from the same native call (csrc/nastar_fastlane.cpp).  The Python lane sorts on
    first use and keeps the order on the hint.  Returns ``start_maps``."""
    lv = levels.reshape(-1)
    if lv.dtype != torch.int32:
        lv = lv.abs().to(torch.int32)
    start_maps.placement_order = OrderHint(None, trusted=True, levels=lv.contiguous())
    return start_maps


def workspace_bytes(shape) -> int:
    """bytes of HBM workspace a [B, H, W] search needs (0: the state of every map lives in LDS)"""
    B, H, W = (int(x) for x in shape[-3:])
    if in_lds(H, W):
        return 0
    return int(_native.load().nastar_workspace_bytes(B, H, W, 0))


def placement_supported(shape) -> bool:
    """sizes ``placement_predict`` handles (csrc/nastar_placement.hip.h)"""
    H, W = int(shape[-2]), int(shape[-1])
    return H == W and W in (32, 64)


def placement_predict(passable: torch.Tensor, start: torch.Tensor, goal: torch.Tensor, return_levels: bool = False):
    """``order`` ([B] int32) for ``astar_forward_ordered`` on a batch that has never been searched: maps sorted, longest first, by the
    length of their shortest 8-connected route over passable cells (include/nastar.h: nastar_placement_predict; two small launches on
    the current stream).  [B,H,W] or [B,1,H,W] fp32 maps, 32x32 or 64x64."""
    _require_device(passable, start, goal)
    lib = _native.load()
    p, s, g = (_maps3(x) for x in (passable, start, goal))
    B, H, W = p.shape
    dev = p.device
    order = torch.empty((B,), dtype=torch.int32, device=dev)
    ws = torch.empty((B,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.nastar_placement_predict(p.data_ptr(), s.data_ptr(), g.data_ptr(), B, H, W, order.data_ptr(), ws.data_ptr(), B * 4, _stream_ptr(dev))
    _native.check(rc, "nastar_placement_predict")
    return (order, ws) if return_levels else order


def new_placement_buffer(B: int, device) -> torch.Tensor:
    """an ``order_out`` buffer for ``astar_forward_ordered``: int32 [B + 1], zeroed (the trailing counter cell must start at 0)"""
    return torch.zeros((B + 1,), dtype=torch.int32, device=device)


def placement_from_iters(iters: torch.Tensor) -> torch.Tensor:
    """an ``order`` for ``astar_forward_ordered`` from known (or predicted) step counts: longest searches first"""
    return torch.argsort(iters, descending=True, stable=True).to(torch.int32)


@torch.library.custom_op("nastar::astar_backward_replay", mutates_args=())
def astar_backward_replay(grad_hist: torch.Tensor, cost: torch.Tensor, start: torch.Tensor, goal: torch.Tensor,
                          passable: torch.Tensor, sel_log: torch.Tensor, g_ratio: float, max_iters: int, iters: torch.Tensor,
                          t_batch: Optional[torch.Tensor], order: Optional[torch.Tensor] = None, flags: int = 0,
                          neighbor_mask: int = NEIGHBORS_MOORE8, heuristic: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dL/dcost by replaying the forward's selection log (csrc/nastar_backward_replay.hip.h): any map size the forward takes
    (1,179,648 cells; 32-bit history stamps above 65519), O(9) accounting work per step.  ``order`` (int32 permutation of 0..B-1): workgroup i replays map order[i] --
    the forward's own completion order (``astar_forward_ordered``'s ``order_out``) puts the longest replays first.  ``flags``:
    ``FLAG_LOCKSTEP`` for the log of an ``exact`` forward (goal selections before the last entry: the general replay loop).
    ``neighbor_mask``: the neighbourhood the forward searched (NEIGHBORS_*; anything but Moore-8: nastar_backward_replay_ordered_masked).
    ``heuristic``: the heuristic maps the forward searched with (nastar_backward_replay_ordered_heuristic); the result is then dL/dheuristic too."""
    _require_device(grad_hist)
    return _replay(cost, start, goal, passable, sel_log, g_ratio, max_iters, iters, t_batch, order, flags, "nastar_backward_replay", grad_hist=grad_hist,
                   neighbor_mask=_mask_arg(neighbor_mask), heuristic=heuristic)


def _replay(cost, start, goal, passable, sel_log, g_ratio, max_iters, iters, t_batch, order, flags, what, *, neighbor_mask=None, heuristic=None,
            multi_source=False, **upstream):
    """body of the two replay ops: allocate dL/dcost and the workspace, issue the call ``replay_call`` assembles.  ``upstream``: the tensors
    of ``replay_call``'s first arguments (grad_hist, or histories / opt_trajs / grad_loss), None where absent"""
    _require_device(cost, start, goal, passable)
    lib = _native.load()
    cost, start, goal, passable, sel_log = (x.contiguous() for x in (cost, start, goal, passable, sel_log))
    upstream = {k: t.contiguous() for k, t in upstream.items() if t is not None}
    B, H, W = cost.shape
    dev = cost.device
    grad_cost = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    ws_bytes = int(lib.nastar_backward_workspace_bytes(B, H, W, int(max_iters)))
    if ws_bytes == 0 and "grad_hist" in upstream:
        raise RuntimeError(f"nastar_backward_replay: unsupported map size {H}x{W}")
    ws = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=dev)
    heuristic = _heuristic_arg(heuristic, cost)
    with torch.cuda.device(dev):
        name, args = replay_call(
            cost=cost.data_ptr(), start=start.data_ptr(), goal=goal.data_ptr(), passable=passable.data_ptr(), sel_log=sel_log.data_ptr(), B=B, H=H,
            W=W, g_ratio=g_ratio, max_iters=max_iters, iters=iters.data_ptr(), t_batch=t_batch.data_ptr() if t_batch is not None else None,
            grad_cost=grad_cost.data_ptr(), workspace=ws.data_ptr(), ws_bytes=ws_bytes, stream=_stream_ptr(dev), flags=flags,
            order=_order_ptr(order, B, dev, True) if order is not None else None, neighbor_mask=neighbor_mask,
            heuristic=heuristic.data_ptr() if heuristic is not None else None, multi_source=multi_source,
            **{k: t.data_ptr() for k, t in upstream.items()})
        rc = getattr(lib, name)(*args)
    _native.check(rc, what)
    return grad_cost


@astar_backward_replay.register_fake
def _(grad_hist, cost, start, goal, passable, sel_log, g_ratio, max_iters, iters, t_batch, order=None, flags=0, neighbor_mask=NEIGHBORS_MOORE8, heuristic=None):
    return torch.empty_like(cost)


_FORWARD_ARGS = tuple(a.name for a in torch.ops.nastar.astar_forward.default._schema.arguments)  # the op's inputs, by name


def _setup_context(ctx, inputs, output):
    a = dict(zip(_FORWARD_ARGS, inputs))
    _, _, iters, _, sel_log = output
    heuristic = a.get("heuristic")  # the heuristic maps the forward searched with: the replay rebuilds its keys from them
    ctx.has_heuristic = heuristic is not None
    saved = [a["cost"], a["start"], a["goal"], a["passable"], iters, sel_log]
    if heuristic is not None:
        saved.append(heuristic)
    ctx.save_for_backward(*saved)
    ctx.g_ratio = a["g_ratio"]
    ctx.max_iters = a["max_iters"]
    ctx.lockstep = bool(a.get("exact", False))  # the log may hold goal selections before its last entry
    ctx.neighbor_mask = int(a.get("neighbor_mask", NEIGHBORS_MOORE8))  # the replay rebuilds the open sets of THIS neighbourhood
    ctx.n_inputs = len(inputs)
    ctx.set_materialize_grads(False)  # no zero-filled gradient tensors for paths / iters / status / sel_log (4 fill launches per step)


def _backward(ctx, g_hist, g_paths, g_iters, g_status, g_log):
    cost, start, goal, passable, iters, sel_log = ctx.saved_tensors[:6]
    heuristic = ctx.saved_tensors[6] if ctx.has_heuristic else None
    grads = [None] * ctx.n_inputs
    if g_hist is None:
        return tuple(grads)
    # t_batch: the reference's batch-wide loop index (differentiable_astar.py:251-255).  BatchCoupling lets the
    # sharded planner substitute the maximum over ALL ranks so gradients match a single-device run.
    t_batch = BatchCoupling.t_batch(iters)
    if sel_log.numel() == 0:
        raise RuntimeError("backward needs the forward's selection log: call astar_forward(..., want_log=True) "
                           "(DifferentiableAstar.forward does whenever cost_maps.requires_grad)")
    grad_cost = torch.ops.nastar.astar_backward_replay(g_hist.contiguous(), cost, start, goal, passable, sel_log,
                                                       ctx.g_ratio, ctx.max_iters, iters, t_batch, None, FLAG_LOCKSTEP if ctx.lockstep else 0,
                                                       ctx.neighbor_mask, heuristic)
    grads[_FORWARD_ARGS.index("cost")] = grad_cost
    if heuristic is not None:
        # dL/dh0 == dL/dcost: g is detached every step (differentiable_astar.py:239), so the loss sees both only through h = h0 + cost
        grads[_FORWARD_ARGS.index("heuristic")] = grad_cost
    return tuple(grads)


astar_forward.register_autograd(_backward, setup_context=_setup_context)


class BatchCoupling:
    """How a map's gradient is coupled to the rest of its batch.

    ``mode``:
      * ``"batch"`` (default, reference semantics): t_batch = max(iters) - 1 over the local batch;
      * ``"none"``: every map is its own batch (no fixed-point terms, shard-size independent);
      * a callable ``iters -> int32 device scalar`` (used by the sharded planner to all-reduce the maximum).
    """

    mode = "batch"

    @classmethod
    def t_batch(cls, iters: torch.Tensor) -> Optional[torch.Tensor]:
        if cls.mode == "none":
            return None
        if callable(cls.mode):
            return cls.mode(iters)
        return (iters.amax() - 1).to(torch.int32).reshape(1)


# ---- training step with the L1 loss fused in (SURVEY.md 8f "next #3"; reference utils/training.py:55-61) ------------------
@torch.library.custom_op("nastar::l1_loss", mutates_args=())
def l1_loss(histories: torch.Tensor, opt_trajs: torch.Tensor) -> torch.Tensor:
    """mean |histories - opt_trajs| as a 1-element device tensor (fixed-order reduction: bitwise reproducible)."""
    _require_device(histories, opt_trajs)
    if histories.shape != opt_trajs.shape:
        raise ValueError(f"shape mismatch {tuple(histories.shape)} vs {tuple(opt_trajs.shape)}")
    lib = _native.load()
    h, t = histories.contiguous(), opt_trajs.contiguous()
    dev = h.device
    out = torch.empty((1,), dtype=torch.float32, device=dev)
    ws = torch.empty((2048,), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = lib.nastar_l1_loss(h.data_ptr(), t.data_ptr(), h.numel(), out.data_ptr(), ws.data_ptr(), 2048, _stream_ptr(dev))
    _native.check(rc, "nastar_l1_loss")
    return out


@l1_loss.register_fake
def _(histories, opt_trajs):
    return histories.new_empty((1,))


@torch.library.custom_op("nastar::astar_backward_l1_replay", mutates_args=())
def astar_backward_l1_replay(histories: torch.Tensor, opt_trajs: torch.Tensor, grad_loss: Optional[torch.Tensor],
                             cost: torch.Tensor, start: torch.Tensor, goal: torch.Tensor, passable: torch.Tensor,
                             sel_log: torch.Tensor, g_ratio: float, max_iters: int, iters: torch.Tensor,
                             t_batch: Optional[torch.Tensor], order: Optional[torch.Tensor] = None, flags: int = 0) -> torch.Tensor:
    """dL/dcost for L = grad_loss * mean|histories - opt_trajs| by replay of the selection log: the sign gradient is formed while the
    upstream values are loaded (no gradient tensor is materialised).  ``flags``: ``FLAG_LOCKSTEP`` for the log of an ``exact`` forward."""
    _require_device(histories, opt_trajs)
    return _replay(cost, start, goal, passable, sel_log, g_ratio, max_iters, iters, t_batch, order, flags, "nastar_backward_l1_replay",
                   histories=histories, opt_trajs=opt_trajs, grad_loss=grad_loss.reshape(1).to(torch.float32) if grad_loss is not None else None)


@astar_backward_l1_replay.register_fake
def _(histories, opt_trajs, grad_loss, cost, start, goal, passable, sel_log, g_ratio, max_iters, iters, t_batch, order=None, flags=0):
    return torch.empty_like(cost)


class _AstarL1Loss(torch.autograd.Function):
    """search + L1 loss as ONE autograd node: forward = nastar_forward_ex + nastar_l1_loss, backward = nastar_backward_l1_replay."""

    @staticmethod
    def forward(ctx, cost, start, goal, passable, opt_trajs, g_ratio, max_iters, order_in, check_order, summary_ptr, exact):
        B = cost.shape[0]
        with torch.no_grad():
            order = None
            if (order_in is not None or B >= PLACEMENT_MIN_BATCH) and workspace_bytes(cost.shape) == 0:
                order = new_placement_buffer(B, cost.device)  # the forward writes the order its searches finish in
                hist, paths, iters, status, sel_log = torch.ops.nastar.astar_forward_ordered(cost, start, goal, passable, g_ratio, max_iters,
                                                                                             True, 0, order_in, order, check_order, summary_ptr, exact)
            else:
                hist, paths, iters, status, sel_log = torch.ops.nastar.astar_forward(cost, start, goal, passable, g_ratio, max_iters, True, 0, summary_ptr,
                                                                                     exact)
            loss = torch.ops.nastar.l1_loss(hist, opt_trajs)
        # (an exact forward may have re-run maps after the launch ranked their completion: the replay then takes the natural order)
        ctx.order = order[:B] if (order is not None and not exact) else None
        ctx.lockstep = bool(exact)
        ctx.save_for_backward(cost, start, goal, passable, opt_trajs, hist, iters, sel_log)
        ctx.g_ratio, ctx.max_iters = g_ratio, max_iters
        ctx.mark_non_differentiable(hist, paths, iters, status)
        ctx.set_materialize_grads(False)  # otherwise autograd zero-fills a gradient for every unused output: 5 fill launches per step
        return loss.reshape(()), hist, paths, iters, status

    @staticmethod
    def backward(ctx, g_loss, g_hist, g_paths, g_iters, g_status):
        cost, start, goal, passable, opt_trajs, hist, iters, sel_log = ctx.saved_tensors
        if g_loss is None:
            return (None,) * 11
        grad_cost = torch.ops.nastar.astar_backward_l1_replay(hist, opt_trajs, g_loss, cost, start, goal, passable, sel_log,
                                                              ctx.g_ratio, ctx.max_iters, iters, BatchCoupling.t_batch(iters), ctx.order,
                                                              FLAG_LOCKSTEP if ctx.lockstep else 0)
        return (grad_cost,) + (None,) * 10


class _AstarForwardPlaced(torch.autograd.Function):
    """``astar_forward`` for large batches under autograd: the forward launch writes the order its searches finish in and the replay
    backward starts its workgroups in that order (same values as the registered autograd of ``astar_forward``; outputs other than
    ``histories`` carry no gradient).  ``order_in`` / ``order_out``: the forward's own placement (planner.Placement / OrderHint) or None."""

    @staticmethod
    def forward(ctx, cost, start, goal, passable, g_ratio, max_iters, flags, order_in, order_out, check_order, summary_ptr, exact):
        B = cost.shape[0]
        with torch.no_grad():
            if order_out is None:
                order_out = new_placement_buffer(B, cost.device)
            hist, paths, iters, status, sel_log = torch.ops.nastar.astar_forward_ordered(cost, start, goal, passable, g_ratio, max_iters, True,
                                                                                         flags, order_in, order_out, check_order, summary_ptr, exact)
        ctx.order = order_out[:B] if not exact else None
        ctx.lockstep = bool(exact)
        ctx.save_for_backward(cost, start, goal, passable, iters, sel_log)
        ctx.g_ratio, ctx.max_iters = g_ratio, max_iters
        ctx.mark_non_differentiable(paths, iters, status, sel_log)
        ctx.set_materialize_grads(False)
        return hist, paths, iters, status, sel_log

    @staticmethod
    def backward(ctx, g_hist, g_paths, g_iters, g_status, g_log):
        if g_hist is None:
            return (None,) * 12
        cost, start, goal, passable, iters, sel_log = ctx.saved_tensors
        grad_cost = torch.ops.nastar.astar_backward_replay(g_hist.contiguous(), cost, start, goal, passable, sel_log, ctx.g_ratio, ctx.max_iters,
                                                           iters, BatchCoupling.t_batch(iters), ctx.order, FLAG_LOCKSTEP if ctx.lockstep else 0)
        return (grad_cost,) + (None,) * 11


class _AstarForwardSources(torch.autograd.Function):
    """the MULTI-SOURCE search under autograd (include/nastar_sources.h): forward = nastar_forward_sources (+ its batch-loop finish when
    ``exact``) with the selection log kept, backward = nastar_backward_replay_sources.  The existing custom ops keep their schemas: this
    node alone carries the flag.  ``heuristic``: [B,H,W] or None; its gradient is the cost's (the loss sees both only through h = h0 + cost)."""

    @staticmethod
    def forward(ctx, cost, start, goal, passable, heuristic, g_ratio, max_iters, summary_ptr, exact, neighbor_mask):
        _require_device(cost, start, goal, passable)
        cost, start, goal, passable = (x.contiguous() for x in (cost, start, goal, passable))
        heuristic = _heuristic_arg(heuristic, cost)
        B, H, W = cost.shape
        with torch.no_grad():
            hist, paths, iters, status, sel_log = _launch_search(_native.load(), cost, start, goal, passable, B, H, W, g_ratio, max_iters, True, 0,
                                                                 cost.device, summary_ptr=summary_ptr, exact=exact, neighbor_mask=neighbor_mask,
                                                                 heuristic=heuristic, multi_source=True)
        ctx.has_heuristic = heuristic is not None
        ctx.save_for_backward(cost, start, goal, passable, iters, sel_log, *((heuristic,) if heuristic is not None else ()))
        ctx.g_ratio, ctx.max_iters, ctx.neighbor_mask = g_ratio, max_iters, neighbor_mask
        ctx.lockstep = bool(exact) and B > 1
        ctx.mark_non_differentiable(paths, iters, status, sel_log)
        ctx.set_materialize_grads(False)
        return hist, paths, iters, status, sel_log

    @staticmethod
    def backward(ctx, g_hist, g_paths, g_iters, g_status, g_log):
        if g_hist is None:
            return (None,) * 10
        cost, start, goal, passable, iters, sel_log = ctx.saved_tensors[:6]
        heuristic = ctx.saved_tensors[6] if ctx.has_heuristic else None
        grad = _replay(cost, start, goal, passable, sel_log, ctx.g_ratio, ctx.max_iters, iters, BatchCoupling.t_batch(iters), None,
                       FLAG_LOCKSTEP if ctx.lockstep else 0, "nastar_backward_replay_sources", neighbor_mask=ctx.neighbor_mask, heuristic=heuristic,
                       multi_source=True, grad_hist=g_hist.contiguous())
        return (grad if ctx.needs_input_grad[0] else None, None, None, None, grad if (ctx.has_heuristic and ctx.needs_input_grad[4]) else None,
                None, None, None, None, None)


def astar_forward_sources(cost, start, goal, passable, g_ratio: float, max_iters: int, heuristic=None, summary_ptr: int = 0, exact: bool = False,
                          neighbor_mask: Optional[int] = None):
    """differentiable multi-source search on [B,H,W] tensors -> (histories, paths, iters, status, sel_log); see ``_AstarForwardSources``"""
    return _AstarForwardSources.apply(cost, start, goal, passable, heuristic, float(g_ratio), int(max_iters), int(summary_ptr), bool(exact),
                                      None if neighbor_mask is None else int(neighbor_mask))


def astar_forward_placed(cost, start, goal, passable, g_ratio: float, max_iters: int, flags: int = 0, order_in=None, order_out=None,
                         check_order: bool = True, summary_ptr: int = 0, exact: bool = False):
    """differentiable ``astar_forward`` (selection log kept) whose backward replays longest-first; see ``_AstarForwardPlaced``"""
    return _AstarForwardPlaced.apply(cost, start, goal, passable, float(g_ratio), int(max_iters), int(flags), order_in, order_out,
                                     bool(check_order), int(summary_ptr), bool(exact))


def astar_l1_loss(cost: torch.Tensor, start: torch.Tensor, goal: torch.Tensor, passable: torch.Tensor,
                  opt_trajs: torch.Tensor, g_ratio: float, max_iters: int, order_in: Optional[torch.Tensor] = None,
                  check_order: bool = True, summary_ptr: int = 0, exact: bool = False):
    """[B,H,W] maps -> (loss scalar, histories, paths, iters, status); only ``loss`` carries gradient (to ``cost``).
    ``order_in``: a placement for the forward launch (``OrderHint.order``); the backward replays by the forward's completion order.
    ``exact``: the reference's batch loop to the letter (``_launch_search``)."""
    return _AstarL1Loss.apply(cost, start, goal, passable, opt_trajs, float(g_ratio), int(max_iters), order_in, bool(check_order), int(summary_ptr),
                              bool(exact))


def heuristic(goal_maps: torch.Tensor) -> torch.Tensor:
    """h0 = get_heuristic(goal_maps) on the device (differentiable_astar.py:26-52); parity/debug helper."""
    _require_device(goal_maps)
    lib = _native.load()
    shape = goal_maps.shape
    g = _maps3(goal_maps)
    B, H, W = g.shape
    out = torch.empty_like(g)
    with torch.cuda.device(g.device):
        rc = lib.nastar_heuristic(g.data_ptr(), B, H, W, out.data_ptr(), _stream_ptr(g.device))
    _native.check(rc, "nastar_heuristic")
    return out.reshape(shape)


# ---- include/nastar_fields.h: the cost-to-go field of whole maps and its optimal policy ----------------------
FIELD_BAD_COST = 9  # NASTAR_ERR_BAD_COST (per-map status of nastar_cost_to_go): a NaN or a negative cost on a passable cell
FIELD_NO_CONVERGENCE = 10  # NASTAR_ERR_NO_CONVERGENCE: the sweep bound was hit (impossible for accepted inputs)
FIELDS_MAX_CELLS = 16384  # nastar_fields_max_cells(): field + cost of one map in the LDS of one workgroup


class FieldOutput(NamedTuple):
    """What ``cost_to_go()`` returns.  ``dists`` [B,1,H,W] fp32: the exact cost to the nearest goal cell from every cell under the search's
    cost semantics (a move costs the cell being LEFT), 0 on goals, +inf on obstacles and where no goal can be reached; ``policies``
    [B,8,H,W] one-hot fp32 (action k = ``utils.synthetic.ACTION_MOVES[k]``: the first move to a neighbour with the smallest distance, if
    that is strictly closer; all-zero on goals, obstacles, unreachable cells and zero-cost plateaus) or None; ``status`` [B] int32: 0, or
    ``STATUS_UNSOLVABLE`` for a map without a goal cell (its field is all +inf)."""

    dists: torch.Tensor
    policies: Optional[torch.Tensor]
    status: torch.Tensor


def _checked_neighbor_mask(neighbor_mask) -> int:
    mask = NEIGHBORS_MOORE8 if neighbor_mask is None else neighbor_mask
    if isinstance(mask, bool) or not isinstance(mask, int) or mask & ~0x1FF or mask & 0x10:
        raise ValueError(f"neighbor_mask must be a 9-bit int with a zero centre bit (include/nastar.h NASTAR_NEIGHBORS_*), got {neighbor_mask!r}")
    return mask


def _field_inputs(cost_maps, goal_maps, obstacles_maps, neighbor_mask):
    """the argument checks ``cost_to_go`` and ``cost_to_go_tiled`` share, in one order: -> (the three maps, the mask, (B, H, W))"""
    maps = (cost_maps, goal_maps, obstacles_maps)
    for name, t in zip(("cost_maps", "goal_maps", "obstacles_maps"), maps):
        if not torch.is_tensor(t) or t.ndim not in (3, 4) or (t.ndim == 4 and t.shape[1] < 1):
            raise ValueError(f"{name} must be a [B,1,H,W] or [B,H,W] tensor, got {tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
        if t.dtype != torch.float32:
            raise TypeError(f"expected float32 maps, got {t.dtype} for {name}")
    shapes = [(t.shape[0],) + tuple(t.shape[-2:]) for t in maps]
    if shapes[1] != shapes[0] or shapes[2] != shapes[0] or min(shapes[0]) < 1:
        raise ValueError(f"cost_maps, goal_maps and obstacles_maps must share one non-empty [B,H,W]: got {shapes[0]}, {shapes[1]}, {shapes[2]}")
    return maps, _checked_neighbor_mask(neighbor_mask), shapes[0]


def _field_device(maps) -> torch.device:
    _require_device(*maps)
    dev = maps[0].device
    if maps[1].device != dev or maps[2].device != dev:
        raise ValueError(f"cost_maps lives on {dev}, goal_maps on {maps[1].device}, obstacles_maps on {maps[2].device}: they must share a device")
    return dev


def _raise_bad_cost(st: torch.Tensor, B: int, what: str) -> None:
    bad = torch.nonzero(st == FIELD_BAD_COST).flatten().tolist()
    if bad:
        raise ValueError(f"{what}: a NaN or a negative cost on a passable cell of map(s) {bad[:16]}{' ...' if len(bad) > 16 else ''} "
                         f"({len(bad)} of {B}); the other maps were computed")


def _raise_plateau(st: torch.Tensor, B: int, what: str) -> None:
    flat = torch.nonzero(st.cpu() == FIELD_PLATEAU).flatten().tolist()
    if flat:
        raise ValueError(f"{what}: a cell with no strictly closer neighbour (a zero-cost plateau) on map(s) {flat[:16]}{' ...' if len(flat) > 16 else ''} "
                         f"({len(flat)} of {B}): the field has no gradient with respect to the costs there; the other maps were computed")


def _raise_no_convergence(st: torch.Tensor, what: str, bound: str) -> None:
    stuck = torch.nonzero(st.cpu() == FIELD_NO_CONVERGENCE).flatten().tolist()
    if stuck:
        raise RuntimeError(f"{what}: map(s) {stuck[:16]} did not converge within {bound} (NASTAR_ERR_NO_CONVERGENCE)")


def _field_lib(symbol: str, header: str):
    """the library, which has to export ``symbol`` of include/``header``"""
    lib = _native.load()
    if not hasattr(lib, symbol):
        raise _native.NativeLibraryMissing(f"{_native.LIB_PATH} is older than include/{header}: rebuild it with `make -C {_native.CSRC_DIR}`")
    return lib


def _check_counts_out(t: Optional[torch.Tensor], name: str, B: int, dev: torch.device) -> None:
    if t is not None and (t.dtype != torch.int32 or t.numel() != B or t.device != dev or not t.is_contiguous()):
        raise ValueError(f"{name} must be a contiguous int32 tensor of {B} elements on {dev}")


def _check_max_rounds(max_rounds) -> None:
    if max_rounds is not None and (isinstance(max_rounds, bool) or not isinstance(max_rounds, int) or max_rounds < 1):
        raise ValueError(f"max_rounds must be a positive int or None, got {max_rounds!r}")


def _check_grad_dists(grad_dists, B: int, H: int, W: int) -> None:
    if not torch.is_tensor(grad_dists) or grad_dists.dtype != torch.float32 or grad_dists.numel() != B * H * W or tuple(grad_dists.shape[-2:]) != (H, W):
        raise ValueError(f"grad_dists must be a float32 tensor of the shape of dists ({B} maps of {H}x{W}), got "
                         f"{tuple(grad_dists.shape) if torch.is_tensor(grad_dists) else type(grad_dists).__name__}")


def _grad_device(maps, grad_dists: torch.Tensor) -> torch.device:
    dev = _field_device(maps)
    _require_device(grad_dists)
    if grad_dists.device != dev:
        raise ValueError(f"dists lives on {dev}, grad_dists on {grad_dists.device}: they must share a device")
    return dev


def _refuse_capture(dev: torch.device, error: type, message: str) -> None:
    with torch.cuda.device(dev):
        capturing = torch.cuda.is_current_stream_capturing()
    if capturing:
        raise error(message)


_BLOCKS = "the call synchronises its stream between batches of rounds and cannot be captured into a graph"


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    """the address of an optional tensor of a C call: None (NULL) for a tensor that is not there"""
    return None if t is None else t.data_ptr()


def _field_outputs(B: int, H: int, W: int, dev: torch.device, policies: bool):
    """what a field call writes -> (dists [B,1,H,W], policies [B,8,H,W] or None, status [B] int32), uninitialised"""
    dists = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)
    pol = torch.empty((B, 8, H, W), dtype=torch.float32, device=dev) if policies else None
    return dists, pol, torch.empty((B,), dtype=torch.int32, device=dev)


def _backward_planes(upstream: Optional[torch.Tensor], B: int, H: int, W: int, dev: torch.device):
    """what a backward call of the family reads and writes -> (the upstream gradient as a contiguous [B,H,W] plane, or None for None;
    grad_cost [B,H,W] and status [B] int32, uninitialised)"""
    up = None if upstream is None else upstream.detach().reshape(B, H, W).contiguous()
    return up, torch.empty((B, H, W), dtype=torch.float32, device=dev), torch.empty((B,), dtype=torch.int32, device=dev)


def _widen_grad(grad: torch.Tensor, shape) -> torch.Tensor:
    """a [B,H,W] gradient in the shape of the ``cost_maps`` it belongs to: of several channels, channel 0 is the cost map (``_maps3``)"""
    if len(shape) == 4 and shape[1] > 1:
        full = grad.new_zeros(shape)
        full[:, 0] = grad
        return full
    return grad.reshape(shape)


def cost_to_go(cost_maps: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor, neighbor_mask: Optional[int] = None,
               policies: bool = True, sweeps_out: Optional[torch.Tensor] = None, tiled: bool = False, differentiable: bool = False) -> FieldOutput:
    """The cost-to-go field of every map of the batch, and the optimal policy that follows it (include/nastar_fields.h).  What follows
    describes the default, ``tiled=False``: one launch, maps of at most ``FIELDS_MAX_CELLS`` cells; see the last sentence for ``tiled=True``.

    ``cost_maps``, ``goal_maps``, ``obstacles_maps``: [B,1,H,W] (or [B,H,W]) float32 on one HIP device; EVERY non-zero cell of a goal map
    is a goal (nearest of K); ``neighbor_mask``: the move set as the search takes it (None = Moore-8).  An evaluation call: no autograd
    graph, detached outputs, on the current stream of the inputs' device.  The per-map status is read before returning (one host
    synchronisation; not inside a hipGraph capture): a NaN or a negative cost on a passable cell raises ValueError naming the rows; a map
    without a goal is reported in ``status``, not raised.  Maps of more than ``FIELDS_MAX_CELLS`` cells raise NotImplementedError.
    ``sweeps_out``: a [B] int32 tensor that receives the sweeps every map's relaxation took (probes).  ``tiled=True`` computes the same
    tensors with ``cost_to_go_tiled`` -- at any map size up to ``FIELDS_TILED_MAX_CELLS``; that call blocks and cannot be captured.

    ``differentiable=True``: the same launch and the same values, and ``dists`` carries an autograd node when ``cost_maps`` requires a
    gradient and grad mode is on (include/nastar_fields_grad.h: its backward is one launch of ``nastar_fields_backward`` on the current
    stream; the gradient goes to ``cost_maps`` alone, in its own shape; ``policies`` and ``status`` are not differentiable).  ``dists``
    holds +inf on obstacles and unreachable cells: a loss masks them itself (``torch.isfinite``); whatever gradient arrives for those
    cells, and for goals, is ignored.  A map with a live cell that has no strictly closer neighbour -- a zero-cost plateau -- has no such
    gradient and raises ValueError naming the rows.  Not with ``tiled=True`` (``cost_to_go_tiled(..., differentiable=True)`` is that call)
    and not inside a stream capture (NotImplementedError)."""
    if differentiable:
        if tiled:
            raise NotImplementedError(f"cost_to_go: differentiable=True is the one-workgroup kernel's (maps of at most {FIELDS_GRAD_MAX_CELLS} cells); "
                                      "the tiled relaxation's backward is cost_to_go_tiled(..., differentiable=True)")
        return _cost_to_go_differentiable(cost_maps, goal_maps, obstacles_maps, neighbor_mask, policies, sweeps_out)
    if tiled:
        if sweeps_out is not None:
            raise ValueError("cost_to_go: sweeps_out belongs to the one-workgroup kernel; cost_to_go_tiled() reports rounds and tile visits")
        return cost_to_go_tiled(cost_maps, goal_maps, obstacles_maps, neighbor_mask=neighbor_mask, policies=policies)[0]
    maps, mask, (B, H, W) = _field_inputs(cost_maps, goal_maps, obstacles_maps, neighbor_mask)
    if H * W > FIELDS_MAX_CELLS:
        raise NotImplementedError(f"cost_to_go: maps of {H}x{W} = {H * W} cells exceed the limit of {FIELDS_MAX_CELLS} cells (one workgroup "
                                  "relaxes one map in LDS; larger maps need a tiled kernel: pass tiled=True)")
    dev = _field_device(maps)
    lib = _field_lib("nastar_cost_to_go", "nastar_fields.h")
    _check_counts_out(sweeps_out, "sweeps_out", B, dev)
    with torch.no_grad():
        cost, goal, passable = (_maps3(t.detach()) for t in maps)
        dists, pol, status = _field_outputs(B, H, W, dev, policies)
        with torch.cuda.device(dev):
            rc = lib.nastar_cost_to_go_sweeps(cost.data_ptr(), goal.data_ptr(), passable.data_ptr(), B, H, W, mask, dists.data_ptr(),
                                              _ptr(pol), status.data_ptr(), _ptr(sweeps_out), _stream_ptr(dev))
        _native.check(rc, "nastar_cost_to_go")
        if not torch.cuda.is_current_stream_capturing():
            st = status.cpu()
            _raise_bad_cost(st, B, "cost_to_go")
            _raise_no_convergence(st, "cost_to_go", "H*W sweeps")
    return FieldOutput(dists, pol, status)


# ---- include/nastar_fields_grad.h: the gradient of that field with respect to the cost maps -------------------
FIELD_PLATEAU = 11  # NASTAR_ERR_PLATEAU (per-map status of nastar_fields_backward): a live cell without a strictly closer neighbour
FIELDS_GRAD_MAX_CELLS = 16384  # nastar_fields_grad_max_cells(): every size nastar_cost_to_go takes


def fields_backward(dists: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor, grad_dists: torch.Tensor,
                    neighbor_mask: Optional[int] = None, sweeps_out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``nastar_fields_backward`` as it is (include/nastar_fields_grad.h): ``dists`` as ``cost_to_go`` returned them, the goal and obstacle
    maps and the mask of that call, and an upstream gradient of ``dists``' shape -> ``(grad_cost [B,H,W], status [B] int32)``.  One launch
    on the current stream, nothing is read back: a map whose status is ``FIELD_PLATEAU`` has an all-zero gradient.  ``grad_dists`` is read
    on live cells only (not a goal, finite distance); ``grad_cost`` is exactly 0 on every other cell.  What ``cost_to_go(...,
    differentiable=True)`` runs in its backward; probes and tests call it directly."""
    maps, mask, (B, H, W) = _field_inputs(dists, goal_maps, obstacles_maps, neighbor_mask)
    _check_grad_dists(grad_dists, B, H, W)
    if H * W > FIELDS_GRAD_MAX_CELLS:
        raise NotImplementedError(f"fields_backward: maps of {H}x{W} = {H * W} cells exceed the limit of {FIELDS_GRAD_MAX_CELLS} cells "
                                  "(larger maps: fields_backward_tiled, or cost_to_go_tiled(..., differentiable=True))")
    dev = _grad_device(maps, grad_dists)
    lib = _field_lib("nastar_fields_backward", "nastar_fields_grad.h")
    _check_counts_out(sweeps_out, "sweeps_out", B, dev)
    with torch.no_grad():
        dist, goal, passable = (_maps3(t.detach()) for t in maps)
        up, grad, status = _backward_planes(grad_dists, B, H, W, dev)
        with torch.cuda.device(dev):
            rc = lib.nastar_fields_backward(dist.data_ptr(), goal.data_ptr(), passable.data_ptr(), up.data_ptr(), B, H, W, mask, grad.data_ptr(),
                                            status.data_ptr(), _ptr(sweeps_out), _stream_ptr(dev))
        _native.check(rc, "nastar_fields_backward")
    return grad, status


class _FieldNode(torch.autograd.Function):
    """A field call as an autograd node, for ``cost_to_go`` and ``cost_to_go_tiled`` alike: ``field(cost, goal, obstacles) -> FieldOutput``
    is the evaluation call (status checks included), ``backward(dists, goal, obstacles, grad_dists) -> grad_cost [B,H,W]`` the raw
    gradient call.  Only ``dists`` carries gradient, and only to ``cost``.  ``taped`` (the soft fields): ``field`` returns ``(output,
    tape)`` and the backward reads the costs again, so both are SAVED beside the other three -- ``cost_maps`` itself, not a copy, under
    autograd's version check -- and the call is ``backward(dists, goal, obstacles, cost, tape, grad_dists)``."""

    @staticmethod
    def forward(ctx, cost_maps, goal_maps, obstacles_maps, field, backward, taped):
        out = field(cost_maps, goal_maps, obstacles_maps)
        kept = ()
        if taped:
            out, tape = out
            kept = (cost_maps, tape)
        ctx.save_for_backward(out.dists, goal_maps, obstacles_maps, *kept)
        ctx.backward_call, ctx.cost_shape = backward, tuple(cost_maps.shape)
        rest = (out.status,) + (() if out.policies is None else (out.policies,))
        ctx.mark_non_differentiable(*rest)
        ctx.set_materialize_grads(False)
        return (out.dists,) + rest

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_dists, *unused):
        if g_dists is None or not ctx.needs_input_grad[0]:
            return (None,) * 6
        grad = ctx.backward_call(*ctx.saved_tensors, g_dists)
        return (_widen_grad(grad, ctx.cost_shape), None, None, None, None, None)


def _differentiable_field(cost_maps, goal_maps, obstacles_maps, field, backward, taped: bool = False) -> FieldOutput:
    """``field(...)``, with the node on ``dists`` when there is something to differentiate"""
    if cost_maps.requires_grad and torch.is_grad_enabled():
        res = _FieldNode.apply(cost_maps, goal_maps, obstacles_maps, field, backward, taped)
        return FieldOutput(res[0], res[2] if len(res) > 2 else None, res[1])
    out = field(cost_maps, goal_maps, obstacles_maps)  # nothing to differentiate: the evaluation call, detached outputs
    return out[0] if taped else out


def _cost_to_go_differentiable(cost_maps, goal_maps, obstacles_maps, neighbor_mask, policies, sweeps_out) -> FieldOutput:
    maps, mask, (B, H, W) = _field_inputs(cost_maps, goal_maps, obstacles_maps, neighbor_mask)
    if H * W > FIELDS_GRAD_MAX_CELLS:
        raise NotImplementedError(f"cost_to_go: differentiable=True takes maps of at most {FIELDS_GRAD_MAX_CELLS} cells, got {H}x{W} = {H * W} "
                                  "(larger maps: cost_to_go_tiled(..., differentiable=True))")
    _refuse_capture(_field_device(maps), NotImplementedError,
                    "cost_to_go: differentiable=True reads the per-map status before it returns and cannot be captured into a graph")
    out = _differentiable_field(cost_maps, goal_maps, obstacles_maps,
                                lambda c, g, o: cost_to_go(c, g, o, neighbor_mask=mask, policies=policies, sweeps_out=sweeps_out),
                                lambda d, g, o, up: fields_backward(d, g, o, up, mask)[0])
    # which maps have no gradient: the backward kernel's own verdict, from a launch with a zero upstream gradient (its set-up and one quiet
    # sweep: a zero gradient is at its fixed point from the start) -- so the rule lives in one place, the kernel, and covers policies=False
    _, st = fields_backward(out.dists.detach(), goal_maps, obstacles_maps, torch.zeros_like(out.dists), mask)
    _raise_plateau(st, B, "cost_to_go")
    return out


# ---- include/nastar_fields_tiled.h: the same field for maps of up to 1179648 cells, by a tiled relaxation ------
FIELDS_TILED_MAX_CELLS = 1179648  # nastar_fields_tiled_max_cells(): the limit of the search entry points


def fields_tile() -> Tuple[int, int]:
    """(rows, columns) of the interior of one tile of ``cost_to_go_tiled`` (nastar_fields_tile)"""
    import ctypes
    th, tw = ctypes.c_int(0), ctypes.c_int(0)
    lib = _field_lib("nastar_cost_to_go_tiled", "nastar_fields_tiled.h")
    _native.check(lib.nastar_fields_tile(ctypes.byref(th), ctypes.byref(tw)), "nastar_fields_tile")
    return th.value, tw.value


def cost_to_go_tiled(cost_maps: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor, neighbor_mask: Optional[int] = None,
                     policies: bool = True, max_rounds: Optional[int] = None, visits_out: Optional[torch.Tensor] = None,
                     launches_per_batch: Optional[int] = None, differentiable: bool = False) -> Tuple[FieldOutput, int]:
    """``cost_to_go`` for maps of up to ``FIELDS_TILED_MAX_CELLS`` cells: the same definition and the same BITS, reached by a tiled
    relaxation (include/nastar_fields_tiled.h) -> ``(FieldOutput, rounds)``.

    The working field lives in ``dists``; a round is one launch in which every active tile relaxes to its local fixed point and marks the
    neighbours that have to look again; rounds are enqueued in batches and the host reads one word per map after each batch.  The call
    therefore BLOCKS on the current stream and is refused while that stream is capturing a graph.  ``rounds``: the rounds in which some
    tile was active.  ``max_rounds=None``: the bound H*W + 1, which no accepted input reaches; status 10 then raises RuntimeError as in
    ``cost_to_go``.  With an explicit ``max_rounds`` a map that still has an active tile is reported in ``status`` (``FIELD_NO_CONVERGENCE``),
    not raised; its ``dists`` are upper bounds of its field, finite only where the field is.  ``visits_out``: a [B] int32 tensor that
    receives every map's (tile, round) visits; ``launches_per_batch``: probes only, not a stable part of the interface (None = the library's choice).

    ``differentiable=True``: the same launches and the same values, and ``dists`` carries an autograd node when ``cost_maps`` requires a
    gradient and grad mode is on (include/nastar_fields_grad_tiled.h).  Its backward is ``fields_backward_tiled`` on the current stream: it
    BLOCKS, like this call, and cannot be captured.  The gradient goes to ``cost_maps`` alone, in its own shape; ``policies`` and
    ``status`` are not differentiable; a loss masks the +inf cells of ``dists`` itself.  A map with a live cell that has no strictly closer
    neighbour -- a zero-cost plateau -- has no such gradient and raises ValueError naming the rows, also when nothing requires a gradient."""
    if differentiable:
        return _cost_to_go_tiled_differentiable(cost_maps, goal_maps, obstacles_maps, neighbor_mask, policies, max_rounds, visits_out, launches_per_batch)
    maps, mask, (B, H, W) = _field_inputs(cost_maps, goal_maps, obstacles_maps, neighbor_mask)
    if H * W > FIELDS_TILED_MAX_CELLS:
        raise NotImplementedError(f"cost_to_go_tiled: maps of {H}x{W} = {H * W} cells exceed the limit of {FIELDS_TILED_MAX_CELLS} cells")
    _check_max_rounds(max_rounds)
    if launches_per_batch is not None and (isinstance(launches_per_batch, bool) or not isinstance(launches_per_batch, int) or launches_per_batch < 1):
        raise ValueError(f"launches_per_batch must be a positive int or None, got {launches_per_batch!r}")
    dev = _field_device(maps)
    lib = _field_lib("nastar_cost_to_go_tiled", "nastar_fields_tiled.h")
    _check_counts_out(visits_out, "visits_out", B, dev)
    _refuse_capture(dev, RuntimeError, f"cost_to_go_tiled: {_BLOCKS}")
    import ctypes
    nbytes = lib.nastar_cost_to_go_tiled_workspace_bytes(B, H, W)
    if nbytes == 0:
        raise NotImplementedError(f"cost_to_go_tiled: a batch of {B} maps of {H}x{W} has more than 2^24 tiles")
    with torch.no_grad():
        cost, goal, passable = (_maps3(t.detach()) for t in maps)
        dists, pol, status = _field_outputs(B, H, W, dev, policies)
        workspace = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        rounds = ctypes.c_int(0)
        with torch.cuda.device(dev):
            rc = lib.nastar_cost_to_go_tiled_batched(cost.data_ptr(), goal.data_ptr(), passable.data_ptr(), B, H, W, mask, dists.data_ptr(),
                                                     _ptr(pol), status.data_ptr(), _ptr(visits_out), workspace.data_ptr(), nbytes,
                                                     0 if max_rounds is None else max_rounds, launches_per_batch or 0,
                                                     ctypes.cast(ctypes.pointer(rounds), ctypes.c_void_p), _stream_ptr(dev))
        _native.check(rc, "nastar_cost_to_go_tiled")
        st = status.cpu()
        _raise_bad_cost(st, B, "cost_to_go_tiled")
        if max_rounds is None:
            _raise_no_convergence(st, "cost_to_go_tiled", "H*W + 1 rounds")
    return FieldOutput(dists, pol, status), rounds.value


# ---- include/nastar_fields_grad_tiled.h: the gradient of the field for maps of up to 1179648 cells, by a tiled subtree sum
FIELDS_GRAD_TILED_MAX_CELLS = 1179648  # nastar_fields_grad_tiled_max_cells(): every size cost_to_go_tiled takes


def _grad_tiled_workspace(lib, B: int, H: int, W: int, dev: torch.device, what: str):
    nbytes = lib.nastar_fields_backward_tiled_workspace_bytes(B, H, W)
    if nbytes == 0:
        raise NotImplementedError(f"{what}: a batch of {B} maps of {H}x{W} has more than 2^24 tiles")
    return torch.empty(((nbytes + 7) // 8,), dtype=torch.float64, device=dev), nbytes  # (fp64 elements: 8-byte aligned whatever the allocator does)


def fields_backward_tiled(dists: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor, grad_dists: torch.Tensor,
                          neighbor_mask: Optional[int] = None, max_rounds: Optional[int] = None,
                          visits_out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, int]:
    """``nastar_fields_backward_tiled`` as it is (include/nastar_fields_grad_tiled.h): ``fields_backward`` for maps of up to
    ``FIELDS_GRAD_TILED_MAX_CELLS`` cells, the same definition and -- on the sizes both take -- the same BITS ->
    ``(grad_cost [B,H,W], status [B] int32, rounds)``.

    ``dists`` as ``cost_to_go`` or ``cost_to_go_tiled`` returned them, the goal and obstacle maps and the mask of that call, an upstream
    gradient of ``dists``' shape, read on live cells only.  The fp64 sums live in a workspace of 9 bytes per cell; a round is one launch in
    which every active tile recomputes itself to its local fixed point and marks the neighbours that have to look again; the host reads
    one word per map after each batch of rounds.  The call therefore BLOCKS on the current stream and is refused (RuntimeError) while that
    stream is capturing a graph, before anything is enqueued.  A map whose status is ``FIELD_PLATEAU`` has an all-zero gradient.
    ``max_rounds=None``: the bound H*W + 1, which no input reaches; status 10 then raises RuntimeError.  With an explicit ``max_rounds`` a
    map that still has an active tile is reported in ``status`` (``FIELD_NO_CONVERGENCE``), not raised, and its gradient is all zero.
    ``visits_out``: a [B] int32 tensor that receives every map's (tile, round) visits."""
    maps, mask, (B, H, W) = _field_inputs(dists, goal_maps, obstacles_maps, neighbor_mask)
    _check_grad_dists(grad_dists, B, H, W)
    if H * W > FIELDS_GRAD_TILED_MAX_CELLS:
        raise NotImplementedError(f"fields_backward_tiled: maps of {H}x{W} = {H * W} cells exceed the limit of {FIELDS_GRAD_TILED_MAX_CELLS} cells")
    _check_max_rounds(max_rounds)
    dev = _grad_device(maps, grad_dists)
    lib = _field_lib("nastar_fields_backward_tiled", "nastar_fields_grad_tiled.h")
    _check_counts_out(visits_out, "visits_out", B, dev)
    _refuse_capture(dev, RuntimeError, f"fields_backward_tiled: {_BLOCKS}")
    import ctypes
    with torch.no_grad():
        workspace, nbytes = _grad_tiled_workspace(lib, B, H, W, dev, "fields_backward_tiled")
        dist, goal, passable = (_maps3(t.detach()) for t in maps)
        up, grad, status = _backward_planes(grad_dists, B, H, W, dev)
        rounds = ctypes.c_int(0)
        with torch.cuda.device(dev):
            rc = lib.nastar_fields_backward_tiled(dist.data_ptr(), goal.data_ptr(), passable.data_ptr(), up.data_ptr(), B, H, W, mask, grad.data_ptr(),
                                                  status.data_ptr(), _ptr(visits_out), workspace.data_ptr(), nbytes, 0 if max_rounds is None else max_rounds,
                                                  ctypes.cast(ctypes.pointer(rounds), ctypes.c_void_p), _stream_ptr(dev))
        _native.check(rc, "nastar_fields_backward_tiled")
        if max_rounds is None:
            _raise_no_convergence(status, "fields_backward_tiled", "H*W + 1 rounds")
    return grad, status, rounds.value


def _fields_plateau_tiled(dists, goal_maps, obstacles_maps, mask) -> torch.Tensor:
    """``nastar_fields_backward_tiled_status``: [B] int32, ``FIELD_PLATEAU`` for the maps without a gradient -- the kernel's own verdict"""
    maps, mask, (B, H, W) = _field_inputs(dists, goal_maps, obstacles_maps, mask)
    dev = _field_device(maps)
    lib = _field_lib("nastar_fields_backward_tiled", "nastar_fields_grad_tiled.h")
    with torch.no_grad():
        workspace, nbytes = _grad_tiled_workspace(lib, B, H, W, dev, "cost_to_go_tiled")
        dist, goal, passable = (_maps3(t.detach()) for t in maps)
        status = torch.empty((B,), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            rc = lib.nastar_fields_backward_tiled_status(dist.data_ptr(), goal.data_ptr(), passable.data_ptr(), B, H, W, mask, status.data_ptr(),
                                                         workspace.data_ptr(), nbytes, _stream_ptr(dev))
        _native.check(rc, "nastar_fields_backward_tiled_status")
    return status


def _cost_to_go_tiled_differentiable(cost_maps, goal_maps, obstacles_maps, neighbor_mask, policies, max_rounds, visits_out, launches_per_batch):
    maps, mask, (B, H, W) = _field_inputs(cost_maps, goal_maps, obstacles_maps, neighbor_mask)
    rounds: list = []

    def field(c, g, o):
        out, n = cost_to_go_tiled(c, g, o, neighbor_mask=mask, policies=policies, max_rounds=max_rounds, visits_out=visits_out,
                                  launches_per_batch=launches_per_batch)
        rounds.append(n)
        return out

    out = _differentiable_field(cost_maps, goal_maps, obstacles_maps, field, lambda d, g, o, up: fields_backward_tiled(d, g, o, up, mask)[0])
    # which maps have no gradient: the backward's own verdict (its init launch and a status write), so the rule lives in one place, the kernel
    _raise_plateau(_fields_plateau_tiled(out.dists.detach(), goal_maps, obstacles_maps, mask), B, "cost_to_go_tiled")
    return out, rounds[0]


# ---- include/nastar_field_routes.h: ordered optimal routes for many start cells per map, read off the field ---
FIELD_ROUTES_MAX_CELLS = 1179648  # nastar_field_routes_max_cells(): every size cost_to_go_tiled takes
FIELD_ROUTES_MAX_QUERIES = 1 << 30  # the most (map, start) pairs one call takes


class FieldRoutes(NamedTuple):
    """What ``field_routes()`` returns, per (map, start) query.  ``routes`` [B,S,L] int32: flat cell indices r*W + c in travel order, the
    goal last, then -1 (``planner.differentiable_astar.route_coords`` turns them into (row, col)); a route longer than L keeps its LAST L
    cells.  ``route_lengths`` [B,S] int32: the true number of route cells.  ``route_costs`` [B,S] fp32: the field at the start cell, +inf
    for an obstacle, an unreachable start and an index outside the map.  ``status`` [B,S] int32: 0, ``STATUS_UNSOLVABLE`` (3: the field
    is not finite at the start), ``FIELD_PLATEAU`` (11: the chain runs into a cell without a strictly closer neighbour) or 1 (the index
    lies outside [0, H*W)); a failed query has length 0 and a row of -1."""

    routes: torch.Tensor
    route_lengths: torch.Tensor
    route_costs: torch.Tensor
    status: torch.Tensor


def _start_indices(starts, B: int, H: int, W: int) -> torch.Tensor:
    """``starts`` of ``field_routes`` -> [B,S] int32 flat indices: an integer [B,S] tensor as it is; a float [B,S,H,W] tensor (the dataset's
    ``start_maps`` layout) by the highest-index non-zero cell of every channel, -1 for an all-zero channel"""
    if not torch.is_tensor(starts) or starts.dtype == torch.bool or starts.is_complex():
        raise TypeError(f"starts must be an integer [B,S] tensor of flat cell indices or a float [B,S,H,W] tensor of start maps, got "
                        f"{starts.dtype if torch.is_tensor(starts) else type(starts).__name__}")
    if starts.is_floating_point():
        if starts.ndim != 4 or starts.shape[0] != B or starts.shape[1] < 1 or tuple(starts.shape[-2:]) != (H, W):
            raise ValueError(f"float starts must be [B,S,H,W] start maps with S >= 1 for {B} maps of {H}x{W}, got {tuple(starts.shape)}")
        cells = torch.arange(1, H * W + 1, dtype=torch.int32, device=starts.device)
        return ((starts.detach().reshape(B, starts.shape[1], H * W) != 0) * cells).amax(-1) - 1
    if starts.ndim != 2 or starts.shape[0] != B or starts.shape[1] < 1:
        raise ValueError(f"integer starts must be [B,S] flat cell indices with S >= 1 for {B} maps, got {tuple(starts.shape)}")
    if starts.dtype == torch.int32:
        return starts.detach()
    return starts.detach().clamp(-1, H * W).to(torch.int32)  # (every index outside the map stays outside it)


def field_routes(dists: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor, starts: torch.Tensor,
                 neighbor_mask: Optional[int] = None, max_route_len: Optional[int] = None) -> FieldRoutes:
    """The ORDERED optimal route from each of S start cells per map to its nearest goal, read off the field (include/nastar_field_routes.h)
    -> ``FieldRoutes``: one field per map answers any number of starts, no search runs.

    ``dists`` as ``cost_to_go`` or ``cost_to_go_tiled`` returned them, the goal and obstacle maps and the mask of that call.  ``starts``:
    an integer [B,S] tensor of flat cell indices r*W + c, or a float [B,S,H,W] tensor in the dataset's ``start_maps`` layout (a channel's
    start is its highest-index non-zero cell; an all-zero channel becomes index -1 and gets status 1).  Maps of up to
    ``FIELD_ROUTES_MAX_CELLS`` cells, at most ``FIELD_ROUTES_MAX_QUERIES`` queries.  An evaluation call on the current stream of the inputs'
    device, detached outputs; nothing raises for a failed query: read ``status``.

    ``max_route_len=L``: one call into the library (a memset of the rows and one launch; two launches above the LDS limit of the table),
    nothing is read back -- it can be captured into a graph; a longer route keeps its last L cells and reports its true length.  ``None``: a lengths-only call, ONE host read of the longest route, then the call that fills
    rows of exactly that length (at least 1); refused while the stream is capturing."""
    maps, mask, (B, H, W) = _field_inputs(dists, goal_maps, obstacles_maps, neighbor_mask)
    idx = _start_indices(starts, B, H, W)
    S = idx.shape[1]
    if max_route_len is not None and (isinstance(max_route_len, bool) or not isinstance(max_route_len, int) or max_route_len < 1):
        raise ValueError(f"max_route_len must be an int >= 1 (or None: the longest route of the call), got {max_route_len!r}")
    if H * W > FIELD_ROUTES_MAX_CELLS:
        raise NotImplementedError(f"field_routes: maps of {H}x{W} = {H * W} cells exceed the limit of {FIELD_ROUTES_MAX_CELLS} cells")
    if B * S > FIELD_ROUTES_MAX_QUERIES:
        raise NotImplementedError(f"field_routes: {B} maps x {S} starts exceed the limit of {FIELD_ROUTES_MAX_QUERIES} queries per call")
    dev = _field_device(maps)
    if idx.device != dev:
        raise ValueError(f"dists lives on {dev}, starts on {idx.device}: they must share a device")
    lib = _field_lib("nastar_field_routes", "nastar_field_routes.h")
    if max_route_len is None:
        _refuse_capture(dev, RuntimeError, "field_routes: max_route_len=None reads the longest route back before it allocates the rows and "
                                           "cannot be captured into a graph; pass max_route_len")
    with torch.no_grad():
        dist, goal, passable = (_maps3(t.detach()) for t in maps)
        idx = idx.contiguous()
        lengths = torch.empty((B, S), dtype=torch.int32, device=dev)
        costs = torch.empty((B, S), dtype=torch.float32, device=dev)
        status = torch.empty((B, S), dtype=torch.int32, device=dev)
        nbytes = lib.nastar_field_routes_workspace_bytes(B, H, W)
        workspace = torch.empty((nbytes,), dtype=torch.uint8, device=dev) if nbytes else None

        def call(routes: Optional[torch.Tensor]) -> None:
            with torch.cuda.device(dev):
                rc = lib.nastar_field_routes(dist.data_ptr(), goal.data_ptr(), passable.data_ptr(), idx.data_ptr(), B, S, H, W, mask,
                                             _ptr(routes), routes.shape[2] if routes is not None else 0,
                                             lengths.data_ptr(), costs.data_ptr(), status.data_ptr(), _ptr(workspace), nbytes, _stream_ptr(dev))
            _native.check(rc, "nastar_field_routes")

        if max_route_len is None:
            call(None)
            max_route_len = max(1, int(lengths.max()))
        routes = torch.empty((B, S, max_route_len), dtype=torch.int32, device=dev)
        call(routes)
    return FieldRoutes(routes, lengths, costs, status)


# ---- include/nastar_path_masks.h: the exact shortest path as a 0/1 mask, and its blackbox gradient -----------
PATH_MASKS_MAX_CELLS = 16384  # nastar_path_masks_max_cells(): the one-workgroup limit of cost_to_go


class PathOutput(NamedTuple):
    """What ``shortest_paths()`` returns.  ``paths`` [B,1,H,W] fp32 0/1: the start, the goal cell reached and every cell of the optimal
    route between them (the convention of ``AstarOutput.paths``); all-zero for a failed map.  ``costs`` [B] fp32: the cost-to-go field at
    the start, the field's own bits (the costs of the cells the route leaves); +inf for a failed map; not differentiable.  ``status`` [B]
    int32: 0, 1 (no start cell), ``STATUS_UNSOLVABLE`` (3: no goal, or the start is an obstacle or cannot reach a goal), ``FIELD_BAD_COST``
    (9), ``FIELD_NO_CONVERGENCE`` (10) or ``FIELD_PLATEAU`` (11: the route runs into a zero-cost plateau)."""

    paths: torch.Tensor
    costs: torch.Tensor
    status: torch.Tensor


def _path_mask_inputs(cost_maps, goal_maps, obstacles_maps, starts, neighbor_mask, what: str, max_cells: Optional[int] = None):
    """the argument checks of the path-mask calls, one-workgroup and tiled (``max_cells``: the tiled limit), in one order -> (the three maps,
    [B] int32 start indices, the mask, (B, H, W), device)"""
    maps, mask, (B, H, W) = _field_inputs(cost_maps, goal_maps, obstacles_maps, neighbor_mask)
    if torch.is_tensor(starts) and starts.is_floating_point() and starts.ndim == 3:
        starts = starts[:, None]
    if not torch.is_tensor(starts) or starts.ndim not in (1, 2, 4) or (starts.ndim > 1 and starts.shape[1] != 1):
        raise ValueError(f"{what}: one start per map -- a [B,1,H,W] (or [B,H,W]) float start map or an integer [B] tensor of flat cell indices, got "
                         f"{tuple(starts.shape) if torch.is_tensor(starts) else type(starts).__name__}")
    idx = _start_indices(starts[:, None] if starts.ndim == 1 else starts, B, H, W).reshape(B)
    if max_cells is not None and H * W > max_cells:
        raise NotImplementedError(f"{what}: maps of {H}x{W} = {H * W} cells exceed the limit of {max_cells} cells")
    if max_cells is None and H * W > PATH_MASKS_MAX_CELLS:
        raise NotImplementedError(f"{what}: maps of {H}x{W} = {H * W} cells exceed the limit of {PATH_MASKS_MAX_CELLS} cells (one workgroup solves "
                                  "one map in LDS; larger maps are shortest_paths_tiled's / path_masks_tiled's)")
    dev = _field_device(maps)
    if idx.device != dev:
        raise ValueError(f"cost_maps lives on {dev}, the starts on {idx.device}: they must share a device")
    return maps, idx.contiguous(), mask, (B, H, W), dev


def _checked_step(value, name: str) -> float:
    """``lambda_`` / ``min_cost``: a finite positive number whose fp32 value and (for lambda_) fp32 reciprocal are finite and positive too"""
    import ctypes
    ok = isinstance(value, (int, float)) and not isinstance(value, bool) and abs(value) < float("inf")
    if ok:
        f = ctypes.c_float(float(value)).value
        ok = 0.0 < f < float("inf") and (name != "lambda_" or ctypes.c_float(1.0 / f).value < float("inf"))
    if not ok:
        raise ValueError(f"{name} must be a finite positive number (in float32 as well), got {value!r}")
    return float(value)


def _check_path_planes(grad_paths, paths_fwd, status_fwd, B: int, H: int, W: int, dev: torch.device) -> None:
    """what a path-mask backward call takes beside the forward's inputs: the upstream gradient, and the forward's paths and status"""
    for name, t in (("grad_paths", grad_paths), ("paths_fwd", paths_fwd)):
        if not torch.is_tensor(t) or t.dtype != torch.float32 or t.numel() != B * H * W or tuple(t.shape[-2:]) != (H, W) or t.device != dev:
            raise ValueError(f"{name} must be a float32 tensor of the shape of the paths ({B} maps of {H}x{W}) on {dev}, got "
                             f"{(tuple(t.shape), t.dtype, t.device) if torch.is_tensor(t) else type(t).__name__}")
    _check_counts_out(status_fwd, "status_fwd", B, dev)
    if status_fwd is None:
        raise ValueError("status_fwd must be the status tensor of the forward call")


def path_masks(cost_maps: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor, starts: torch.Tensor,
               neighbor_mask: Optional[int] = None) -> PathOutput:
    """``nastar_path_masks`` as it is (include/nastar_path_masks.h): one launch on the current stream, nothing is read back and nothing
    raises for a failed map -- read ``status``.  ``starts``: a float [B,1,H,W] start map (its highest-index non-zero cell) or an integer
    [B] tensor of flat cell indices.  Detached outputs.  What ``shortest_paths`` runs; probes and tests call it directly."""
    maps, idx, mask, (B, H, W), dev = _path_mask_inputs(cost_maps, goal_maps, obstacles_maps, starts, neighbor_mask, "path_masks")
    lib = _field_lib("nastar_path_masks", "nastar_path_masks.h")
    with torch.no_grad():
        cost, goal, passable = (_maps3(t.detach()) for t in maps)
        paths = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)
        costs = torch.empty((B,), dtype=torch.float32, device=dev)
        status = torch.empty((B,), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            rc = lib.nastar_path_masks(cost.data_ptr(), goal.data_ptr(), passable.data_ptr(), idx.data_ptr(), B, H, W, mask, paths.data_ptr(),
                                       costs.data_ptr(), status.data_ptr(), _stream_ptr(dev))
        _native.check(rc, "nastar_path_masks")
    return PathOutput(paths, costs, status)


def path_masks_backward(cost_maps: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor, starts: torch.Tensor,
                        grad_paths: torch.Tensor, paths_fwd: torch.Tensor, status_fwd: torch.Tensor, lambda_: float, min_cost: float = 2.0 ** -10,
                        neighbor_mask: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``nastar_path_masks_backward`` as it is: the inputs of ``path_masks``, the upstream gradient of ``paths``, and ``paths`` and
    ``status`` as that call returned them -> ``(grad_cost [B,H,W], status [B] int32 of the perturbed solve)``.  One launch on the current
    stream, nothing is read back.  ``grad_cost`` is 0 or +-fl32(1/lambda_) per cell; all-zero for a map whose ``status_fwd`` is not 0,
    all-NaN for a map whose perturbed solve failed.  What the backward of ``shortest_paths(..., lambda_=...)`` runs."""
    lam, floor = _checked_step(lambda_, "lambda_"), _checked_step(min_cost, "min_cost")
    maps, idx, mask, (B, H, W), dev = _path_mask_inputs(cost_maps, goal_maps, obstacles_maps, starts, neighbor_mask, "path_masks_backward")
    _check_path_planes(grad_paths, paths_fwd, status_fwd, B, H, W, dev)
    lib = _field_lib("nastar_path_masks_backward", "nastar_path_masks.h")
    with torch.no_grad():
        cost, goal, passable = (_maps3(t.detach()) for t in maps)
        up, grad, status = _backward_planes(grad_paths, B, H, W, dev)
        fwd = paths_fwd.detach().reshape(B, H, W).contiguous()
        with torch.cuda.device(dev):
            rc = lib.nastar_path_masks_backward(cost.data_ptr(), goal.data_ptr(), passable.data_ptr(), idx.data_ptr(), up.data_ptr(), fwd.data_ptr(),
                                                status_fwd.data_ptr(), B, H, W, mask, lam, floor, grad.data_ptr(), status.data_ptr(), _stream_ptr(dev))
        _native.check(rc, "nastar_path_masks_backward")
    return grad, status


class _PathNode(torch.autograd.Function):
    """``path_masks`` as an autograd node: only ``paths`` carries gradient, and only to ``cost_maps`` -- the blackbox gradient, one launch of
    ``path_masks_backward`` on the current stream, no host read.  ``tiled``: ``path_masks_tiled`` and ``path_masks_tiled_backward`` in their
    place -- both block."""

    @staticmethod
    def forward(ctx, cost_maps, goal_maps, obstacles_maps, idx, mask, lam, floor, tiled):
        out = (path_masks_tiled if tiled else path_masks)(cost_maps, goal_maps, obstacles_maps, idx, mask)
        ctx.save_for_backward(cost_maps, goal_maps, obstacles_maps, idx, out.paths, out.status)
        ctx.step, ctx.cost_shape, ctx.tiled = (mask, lam, floor), tuple(cost_maps.shape), tiled
        ctx.mark_non_differentiable(out.costs, out.status)
        ctx.set_materialize_grads(False)
        return out.paths, out.costs, out.status

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_paths, *unused):
        if g_paths is None or not ctx.needs_input_grad[0]:
            return (None,) * 8
        cost, goal, obstacles, idx, paths, status = ctx.saved_tensors
        mask, lam, floor = ctx.step
        grad, _ = (path_masks_tiled_backward if ctx.tiled else path_masks_backward)(cost, goal, obstacles, idx, g_paths, paths, status, lam, floor, mask)
        return (_widen_grad(grad, ctx.cost_shape),) + (None,) * 7


def _raise_path_failures(status: torch.Tensor, B: int, what: str, bound: str, differentiable: bool) -> None:
    """the one status read of ``shortest_paths`` / ``shortest_paths_tiled``: a bad cost and a relaxation that hit its bound raise; with a
    gradient asked for, so does a plateau"""
    st = status.cpu()
    _raise_bad_cost(st, B, what)
    _raise_no_convergence(st, what, bound)
    flat = torch.nonzero(st == FIELD_PLATEAU).flatten().tolist()
    if differentiable and flat:
        raise ValueError(f"{what}: the route of map(s) {flat[:16]}{' ...' if len(flat) > 16 else ''} ({len(flat)} of {B}) runs into a cell "
                         "with no strictly closer neighbour (a zero-cost plateau): no path, so no gradient; the other maps were computed")


def shortest_paths(cost_maps: torch.Tensor, start_maps: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor,
                   neighbor_mask: Optional[int] = None, lambda_: Optional[float] = None, min_cost: float = 2.0 ** -10) -> PathOutput:
    """The EXACT optimal path of every map as a 0/1 mask, as a layer (include/nastar_path_masks.h) -> ``PathOutput``: the cost-to-go field
    of ``cost_to_go`` and the route of ``field_routes`` in ONE launch, no field or policy plane in memory.  A move costs the cell being
    left; ``g_ratio``, ``Tmax`` and the heuristic play no part: unlike a search with costs below 1, the path IS the minimiser.

    ``cost_maps``, ``start_maps``, ``goal_maps``, ``obstacles_maps``: [B,1,H,W] (or [B,H,W]) float32 on one HIP device, maps of at most
    ``PATH_MASKS_MAX_CELLS`` cells (NotImplementedError above).  ``start_maps`` is one-hot; of several non-zero cells the one with the
    highest flat index is the start (the search's own default rule); an all-zero map gets status 1.  Every non-zero cell of a goal map is a
    goal (the nearest one is reached).  ``neighbor_mask``: the move set as the search takes it (None = Moore-8).

    ``lambda_=None``: an evaluation call -- detached outputs, one host read for the status (none inside a stream capture): a NaN or a
    negative cost on a passable cell raises ValueError naming the rows; every other failure stays in ``status``.

    ``lambda_`` a positive float: ``paths`` carries an autograd node when ``cost_maps`` requires a gradient (blackbox differentiation of
    the solver, Vlastelica et al. 2020).  Its backward is ONE launch and reads nothing back: with g = dL/dpaths it solves the costs
    ``max(fl32(fl32(lambda_ * g) + cost), min_cost)`` and returns ``(paths_lambda - paths) * fl32(1 / lambda_)`` -- 0 or +-1/lambda_ per
    cell -- to ``cost_maps`` alone.  The forward reads the status once (not inside a capture) and raises ValueError for rows with a bad
    cost or a plateau; a map that failed otherwise (see ``status``) gets a zero gradient; a map whose PERTURBED solve fails (a NaN in g)
    gets an all-NaN gradient row.  ``lambda_`` trades the informativeness of the gradient against its faithfulness and is the user's to
    choose (the blackbox paper uses 20 on WarCraft costs); ``min_cost``, the floor of the perturbed costs, is an API default chosen so
    that a clamped cell stays strictly positive -- 2^-10 is NOT a tuned number.

    Zero costs: a route that would run through a zero-cost plateau (no strictly closer neighbour) has no defined successor and is reported
    as ``FIELD_PLATEAU``.  The same holds in float32 for very small costs on long routes: where ``fl32(c + D) == D`` the field does not
    fall along the move, which is a plateau in the sense of the field rules and is reported as such."""
    differentiable = lambda_ is not None
    if differentiable:
        lam = _checked_step(lambda_, "lambda_")
    floor = _checked_step(min_cost, "min_cost")
    maps, idx, mask, (B, H, W), dev = _path_mask_inputs(cost_maps, goal_maps, obstacles_maps, start_maps, neighbor_mask, "shortest_paths")
    if differentiable and cost_maps.requires_grad and torch.is_grad_enabled():
        out = PathOutput(*_PathNode.apply(cost_maps, goal_maps, obstacles_maps, idx, mask, lam, floor, False))
    else:
        out = path_masks(cost_maps, goal_maps, obstacles_maps, idx, mask)
    with torch.cuda.device(dev):
        capturing = torch.cuda.is_current_stream_capturing()
    if not capturing:
        _raise_path_failures(out.status, B, "shortest_paths", "H*W sweeps", differentiable)
    return out


# ---- include/nastar_path_masks_tiled.h: that mask and that gradient for maps of up to 1179648 cells ------------
PATH_MASKS_TILED_MAX_CELLS = 1179648  # nastar_path_masks_tiled_max_cells(): every size cost_to_go_tiled takes


def _path_tiled_workspace(lib, backward: bool, B: int, H: int, W: int, dev: torch.device, what: str):
    sizer = lib.nastar_path_masks_tiled_backward_workspace_bytes if backward else lib.nastar_path_masks_tiled_workspace_bytes
    nbytes = sizer(B, H, W)
    if nbytes == 0:
        raise NotImplementedError(f"{what}: a batch of {B} maps of {H}x{W} has more than 2^24 tiles")
    return torch.empty(((nbytes + 3) // 4,), dtype=torch.int32, device=dev), nbytes  # (int32 elements: 4-byte aligned whatever the allocator does)


def path_masks_tiled(cost_maps: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor, starts: torch.Tensor,
                     neighbor_mask: Optional[int] = None, max_rounds: Optional[int] = None, return_rounds: bool = False):
    """``nastar_path_masks_tiled`` as it is (include/nastar_path_masks_tiled.h): ``path_masks`` for maps of up to
    ``PATH_MASKS_TILED_MAX_CELLS`` cells, the same definition and -- on the sizes both take -- the same BITS -> ``PathOutput``, or
    ``(PathOutput, rounds)`` with ``return_rounds=True`` (the rounds of the relaxation in which some tile was active).

    The field is ``cost_to_go_tiled``'s, written into a workspace this call allocates (4 bytes per cell and the relaxation's own words);
    one more launch turns it into the mask.  The relaxation synchronises its stream between batches of rounds: the call BLOCKS and is
    refused (RuntimeError) while that stream is capturing a graph, before anything is enqueued.  Nothing raises for a failed map -- read
    ``status``.  ``max_rounds=None``: the bound H*W + 1, which no accepted input reaches; with an explicit ``max_rounds`` a map that still
    has an active tile gets ``FIELD_NO_CONVERGENCE``, a zero mask and a cost of +inf.  Detached outputs."""
    _check_max_rounds(max_rounds)
    maps, idx, mask, (B, H, W), dev = _path_mask_inputs(cost_maps, goal_maps, obstacles_maps, starts, neighbor_mask, "path_masks_tiled",
                                                        PATH_MASKS_TILED_MAX_CELLS)
    lib = _field_lib("nastar_path_masks_tiled", "nastar_path_masks_tiled.h")
    _refuse_capture(dev, RuntimeError, f"path_masks_tiled: {_BLOCKS}")
    import ctypes
    with torch.no_grad():
        workspace, nbytes = _path_tiled_workspace(lib, False, B, H, W, dev, "path_masks_tiled")
        cost, goal, passable = (_maps3(t.detach()) for t in maps)
        paths = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)
        costs = torch.empty((B,), dtype=torch.float32, device=dev)
        status = torch.empty((B,), dtype=torch.int32, device=dev)
        rounds = ctypes.c_int(0)
        with torch.cuda.device(dev):
            rc = lib.nastar_path_masks_tiled(cost.data_ptr(), goal.data_ptr(), passable.data_ptr(), idx.data_ptr(), B, H, W, mask, paths.data_ptr(),
                                             costs.data_ptr(), status.data_ptr(), workspace.data_ptr(), nbytes, 0 if max_rounds is None else max_rounds,
                                             ctypes.cast(ctypes.pointer(rounds), ctypes.c_void_p), _stream_ptr(dev))
        _native.check(rc, "nastar_path_masks_tiled")
    out = PathOutput(paths, costs, status)
    return (out, rounds.value) if return_rounds else out


def path_masks_tiled_backward(cost_maps: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor, starts: torch.Tensor,
                              grad_paths: torch.Tensor, paths_fwd: torch.Tensor, status_fwd: torch.Tensor, lambda_: float,
                              min_cost: float = 2.0 ** -10, neighbor_mask: Optional[int] = None, max_rounds: Optional[int] = None,
                              return_rounds: bool = False):
    """``nastar_path_masks_tiled_backward`` as it is: ``path_masks_backward`` for maps of up to ``PATH_MASKS_TILED_MAX_CELLS`` cells, the
    same definition and -- on the sizes both take -- the same BITS -> ``(grad_cost [B,H,W], status [B] int32 of the perturbed solve)``, and
    the rounds of the perturbed relaxation as a third element with ``return_rounds=True``.  One elementwise launch writes the perturbed
    costs into the workspace, ``cost_to_go_tiled``'s relaxation solves them, one launch writes the rows.  The call BLOCKS and is refused
    (RuntimeError) while its stream is capturing.  ``grad_cost`` is all-zero for a map whose ``status_fwd`` is not 0 (the map is relaxed
    with the batch all the same; its field is not looked at), all-NaN for a map whose perturbed solve failed -- a map cut short by an
    explicit ``max_rounds`` among them (``FIELD_NO_CONVERGENCE``).  What the backward of ``shortest_paths_tiled(..., lambda_=...)`` runs."""
    lam, floor = _checked_step(lambda_, "lambda_"), _checked_step(min_cost, "min_cost")
    _check_max_rounds(max_rounds)
    maps, idx, mask, (B, H, W), dev = _path_mask_inputs(cost_maps, goal_maps, obstacles_maps, starts, neighbor_mask, "path_masks_tiled_backward",
                                                        PATH_MASKS_TILED_MAX_CELLS)
    _check_path_planes(grad_paths, paths_fwd, status_fwd, B, H, W, dev)
    lib = _field_lib("nastar_path_masks_tiled_backward", "nastar_path_masks_tiled.h")
    _refuse_capture(dev, RuntimeError, f"path_masks_tiled_backward: {_BLOCKS}")
    import ctypes
    with torch.no_grad():
        workspace, nbytes = _path_tiled_workspace(lib, True, B, H, W, dev, "path_masks_tiled_backward")
        cost, goal, passable = (_maps3(t.detach()) for t in maps)
        up, grad, status = _backward_planes(grad_paths, B, H, W, dev)
        fwd = paths_fwd.detach().reshape(B, H, W).contiguous()
        rounds = ctypes.c_int(0)
        with torch.cuda.device(dev):
            rc = lib.nastar_path_masks_tiled_backward(cost.data_ptr(), goal.data_ptr(), passable.data_ptr(), idx.data_ptr(), up.data_ptr(),
                                                      fwd.data_ptr(), status_fwd.data_ptr(), B, H, W, mask, lam, floor, grad.data_ptr(),
                                                      status.data_ptr(), workspace.data_ptr(), nbytes, 0 if max_rounds is None else max_rounds,
                                                      ctypes.cast(ctypes.pointer(rounds), ctypes.c_void_p), _stream_ptr(dev))
        _native.check(rc, "nastar_path_masks_tiled_backward")
    return (grad, status, rounds.value) if return_rounds else (grad, status)


def shortest_paths_tiled(cost_maps: torch.Tensor, start_maps: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor,
                         neighbor_mask: Optional[int] = None, lambda_: Optional[float] = None, min_cost: float = 2.0 ** -10) -> PathOutput:
    """``shortest_paths`` for maps of up to ``PATH_MASKS_TILED_MAX_CELLS`` cells (include/nastar_path_masks_tiled.h) -> ``PathOutput``: the
    same definition, the same arguments, the same conventions for failed maps and -- on the sizes both take -- the same BITS, forward and
    backward.  The contract is that of ``shortest_paths`` with three differences.  The limit is ``PATH_MASKS_TILED_MAX_CELLS`` cells
    (NotImplementedError above).  The field comes from the tiled relaxation of ``cost_to_go_tiled``, which synchronises its stream between
    batches of rounds: the call BLOCKS and raises RuntimeError inside a stream capture, before any launch.  And with ``lambda_`` the
    backward of the autograd node on ``paths`` -- one elementwise launch, the same relaxation on the perturbed costs, one launch for the
    rows -- blocks too.  The status is always read once: a NaN or a negative cost on a passable cell raises ValueError naming the rows, and
    so does, with ``lambda_``, a route that runs into a zero-cost plateau; every other failure stays in ``status``.  ``min_cost`` is an API
    default, NOT a tuned number."""
    differentiable = lambda_ is not None
    if differentiable:
        lam = _checked_step(lambda_, "lambda_")
    _checked_step(min_cost, "min_cost")
    floor = float(min_cost)
    maps, idx, mask, (B, H, W), dev = _path_mask_inputs(cost_maps, goal_maps, obstacles_maps, start_maps, neighbor_mask, "shortest_paths_tiled",
                                                        PATH_MASKS_TILED_MAX_CELLS)
    _refuse_capture(dev, RuntimeError, f"shortest_paths_tiled: {_BLOCKS}")
    if differentiable and cost_maps.requires_grad and torch.is_grad_enabled():
        out = PathOutput(*_PathNode.apply(cost_maps, goal_maps, obstacles_maps, idx, mask, lam, floor, True))
    else:
        out = path_masks_tiled(cost_maps, goal_maps, obstacles_maps, idx, mask)
    _raise_path_failures(out.status, B, "shortest_paths_tiled", "H*W + 1 rounds", differentiable)
    return out


# ---- include/nastar_soft_fields.h: the entropy-regularised cost-to-go field over a finite horizon and its gradient
SOFT_FIELDS_MAX_CELLS = 12288  # nastar_soft_fields_max_cells(): the cost and two planes of one map in the LDS of one workgroup
SOFT_FIELDS_GRAD_MAX_CELLS = 6144  # nastar_soft_fields_grad_max_cells(): the backward keeps 25 bytes per cell


class SoftFieldOutput(NamedTuple):
    """What ``soft_cost_to_go()`` returns.  ``dists`` [B,1,H,W] fp32: the soft-min cost-to-go V_K (0 on goals, +inf on obstacles and where
    no goal lies within ``horizon`` moves); ``policies`` [B,8,H,W] fp32 (action k = ``utils.synthetic.ACTION_MOVES[k]``: the softmax over
    the allowed moves with a finite target of -V_{K-1} / tau; all-zero on goals, obstacles and cells with an infinite ``dists``), detached,
    or None; ``status`` [B] int32: 0, or ``STATUS_UNSOLVABLE`` for a map without a goal cell."""

    dists: torch.Tensor
    policies: Optional[torch.Tensor]
    status: torch.Tensor


def _checked_tau(tau) -> float:
    if isinstance(tau, bool) or not isinstance(tau, (int, float)) or not 0.0 < float(tau) < float("inf"):
        raise ValueError(f"tau must be a finite positive Python float (the temperature; it has no gradient), got {tau!r}")
    return float(tau)


def _checked_horizon(horizon, H: int, W: int) -> int:
    if horizon is None:
        return 2 * (H + W)
    if isinstance(horizon, bool) or not isinstance(horizon, int) or not 1 <= horizon < 2 ** 31:
        raise ValueError(f"horizon must be a positive int or None (= 2 * (H + W)), got {horizon!r}")
    return horizon


# The four headers of the family by (tiled, log-policy): the header, its forward and its backward entry point -- each variant calls ITS
# OWN: they are other kernel instantiations, and the field's are not the policy's with a NULL pointer -- and the names its refusals carry:
# the public call in the forward's, the stem of ``<stem>_forward`` / ``<stem>_backward`` in the backward's.
_SOFT_VARIANTS = {
    (False, False): ("nastar_soft_fields.h", "nastar_soft_cost_to_go", "nastar_soft_fields_backward", "soft_cost_to_go", "soft_fields"),
    (True, False): ("nastar_soft_fields_tiled.h", "nastar_soft_cost_to_go_tiled", "nastar_soft_fields_backward_tiled", "soft_cost_to_go_tiled",
                    "soft_fields_tiled"),
    (False, True): ("nastar_soft_policy.h", "nastar_soft_policy_forward", "nastar_soft_policy_backward", "soft_policy", "soft_policy"),
    (True, True): ("nastar_soft_policy_tiled.h", "nastar_soft_policy_forward_tiled", "nastar_soft_policy_backward_tiled", "soft_policy_tiled",
                   "soft_policy_tiled"),
}


def _soft_forward(tiled: bool, logp: bool, cost_maps, goal_maps, obstacles_maps, tau, horizon, neighbor_mask, policies: bool, tape: bool,
                  checkpoint_every=None, sweeps_per_launch=None, tape_limit: Optional[int] = None):
    """the raw forward call of the four variants: the refusals in the family's one order, the outputs, ONE C call with its arguments in
    header order -> ``(dists, log_policies or None, policies or None, status, tape or None)``.  ``logp``: the log-policy beside the
    other outputs; ``tiled``: ``checkpoint_every``, ``sweeps_per_launch`` and a workspace, which the one-workgroup call does not have.
    ``tape_limit``: the largest map a one-workgroup call with a tape takes, None = the backward's (``soft_routes`` reads every size)."""
    header, symbol, _, what, _ = _SOFT_VARIANTS[tiled, logp]
    t = _checked_tau(tau)
    maps, mask, (B, H, W) = _field_inputs(cost_maps, goal_maps, obstacles_maps, neighbor_mask)
    K = _checked_horizon(horizon, H, W)
    if tiled:
        c = _checked_checkpoint_every(checkpoint_every, K)
        if sweeps_per_launch is not None and (isinstance(sweeps_per_launch, bool) or not isinstance(sweeps_per_launch, int) or sweeps_per_launch < 1):
            raise ValueError(f"sweeps_per_launch must be a positive int or None, got {sweeps_per_launch!r}")
        _soft_tiled_limit(H, W, what)
    else:
        # (a tape is for the backward, which takes fewer cells than the forward -- unless the caller reads it itself: ``tape_limit``)
        limit = (SOFT_FIELDS_GRAD_MAX_CELLS if tape_limit is None else tape_limit) if tape else SOFT_FIELDS_MAX_CELLS
        if H * W > limit:
            raise NotImplementedError(f"{what}: maps of {H}x{W} = {H * W} cells exceed the limit of {limit} cells{' of its backward' if tape else ''} "
                                      f"(one workgroup keeps one map in LDS{'' if logp else '; larger maps: soft_cost_to_go_tiled'})")
    dev = _field_device(maps)
    lib = _field_lib(symbol, header)
    with torch.no_grad():
        cost, goal, passable = (_maps3(m.detach()) for m in maps)
        dists, pol, status = _field_outputs(B, H, W, dev, policies)
        log_pol = torch.empty((B, 8, H, W), dtype=torch.float32, device=dev) if logp else None
        tape_bytes = 0
        if tape:
            tape_bytes = int(lib.nastar_soft_fields_tiled_tape_bytes(B, H, W, K, c) if tiled else lib.nastar_soft_fields_tape_bytes(B, H, W, K))
        buf = torch.empty((tape_bytes,), dtype=torch.uint8, device=dev) if tape else None
        args = (cost.data_ptr(), goal.data_ptr(), passable.data_ptr(), B, H, W, mask, t, K, dists.data_ptr(), _ptr(pol))
        if logp:
            args += (log_pol.data_ptr(),)
        args += (status.data_ptr(), _ptr(buf), tape_bytes)
        entry = symbol
        if tiled:
            ws_bytes = int(lib.nastar_soft_fields_tiled_workspace_bytes(B, H, W))
            ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
            args += (c, ws.data_ptr(), ws_bytes)
            if sweeps_per_launch is not None:  # nastar_soft_cost_to_go_tiled_with_sweeps / nastar_soft_policy_forward_tiled_with_sweeps
                entry, args = symbol + "_with_sweeps", args + (sweeps_per_launch,)
        with torch.cuda.device(dev):
            rc = getattr(lib, entry)(*args, _stream_ptr(dev))
        _native.check(rc, symbol)
    return dists, log_pol, pol, status, buf


def _soft_backward(tiled: bool, logp: bool, cost_maps, goal_maps, obstacles_maps, tape, grad_dists, grad_log_policies, tau, horizon, neighbor_mask,
                   checkpoint_every=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """the raw backward call of the four variants, as ``_soft_forward`` is their forward -> ``(grad_cost [B,H,W], status [B] int32)``.
    ``logp``: a second upstream gradient, and either may be None; without it ``grad_dists`` is required (``grad_log_policies`` is not
    looked at).  ``tiled``: ``checkpoint_every`` and a workspace of the variant's own size."""
    header, _, symbol, _, name = _SOFT_VARIANTS[tiled, logp]
    t = _checked_tau(tau)
    maps, mask, (B, H, W) = _field_inputs(cost_maps, goal_maps, obstacles_maps, neighbor_mask)
    K = _checked_horizon(horizon, H, W)
    if tiled:
        c = _checked_checkpoint_every(checkpoint_every, K)
    if grad_dists is not None or not logp:
        _check_grad_dists(grad_dists, B, H, W)
    if logp and grad_log_policies is not None and (not torch.is_tensor(grad_log_policies) or grad_log_policies.dtype != torch.float32
                                                   or tuple(grad_log_policies.shape) != (B, 8, H, W)):
        raise ValueError(f"grad_log_policies must be a float32 tensor of the shape of log_policies ({B}, 8, {H}, {W}), got "
                         f"{tuple(grad_log_policies.shape) if torch.is_tensor(grad_log_policies) else type(grad_log_policies).__name__}")
    if tiled:
        _soft_tiled_limit(H, W, f"{name}_backward")
    elif H * W > SOFT_FIELDS_GRAD_MAX_CELLS:
        raise NotImplementedError(f"{name}_backward: maps of {H}x{W} = {H * W} cells exceed the limit of {SOFT_FIELDS_GRAD_MAX_CELLS} cells")
    if logp:
        dev = _field_device(maps)
        for which, g in (("grad_dists", grad_dists), ("grad_log_policies", grad_log_policies)):
            if g is not None and g.device != dev:
                raise ValueError(f"the maps live on {dev}, {which} on {g.device}: they must share a device")
    else:
        dev = _grad_device(maps, grad_dists)
    lib = _field_lib(symbol, header)
    if not torch.is_tensor(tape) or tape.dtype != torch.uint8 or tape.device != dev or not tape.is_contiguous():
        raise ValueError(f"tape must be the contiguous uint8 tensor {name}_forward(..., tape=True) returned, on {dev}")
    with torch.no_grad():
        cost, goal, passable = (_maps3(m.detach()) for m in maps)
        up, grad, status = _backward_planes(grad_dists, B, H, W, dev)
        args = (cost.data_ptr(), goal.data_ptr(), passable.data_ptr(), tape.data_ptr(), tape.numel()) + ((c,) if tiled else ()) + (_ptr(up),)
        if logp:
            upl = None if grad_log_policies is None else grad_log_policies.detach().contiguous()  # (named: it lives until the call is enqueued)
            args += (_ptr(upl),)
        args += (B, H, W, mask, t, K, grad.data_ptr(), status.data_ptr())
        if tiled:
            sizer = lib.nastar_soft_policy_tiled_backward_workspace_bytes if logp else lib.nastar_soft_fields_tiled_backward_workspace_bytes
            ws_bytes = int(sizer(B, H, W, K, c))
            ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
            args += (ws.data_ptr(), ws_bytes)
        with torch.cuda.device(dev):
            rc = getattr(lib, symbol)(*args, _stream_ptr(dev))
        _native.check(rc, symbol)
    return grad, status


def soft_fields_forward(cost_maps: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor, tau: float, horizon: Optional[int] = None,
                        neighbor_mask: Optional[int] = None, policies: bool = False, tape: bool = False):
    """``nastar_soft_cost_to_go`` as it is (include/nastar_soft_fields.h) -> ``(SoftFieldOutput, tape)``: one launch on the current stream,
    nothing is read back, detached outputs.  ``tape=True`` allocates the tape of ``nastar_soft_fields_tape_bytes`` bytes (the planes
    V_1 .. V_K, what ``soft_fields_backward`` reads) and returns it as a uint8 tensor; None otherwise.  What ``soft_cost_to_go`` runs;
    probes and tests call it directly."""
    dists, _, pol, status, buf = _soft_forward(False, False, cost_maps, goal_maps, obstacles_maps, tau, horizon, neighbor_mask, policies, tape)
    return SoftFieldOutput(dists, pol, status), buf


def soft_fields_backward(cost_maps: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor, tape: torch.Tensor,
                         grad_dists: torch.Tensor, tau: float, horizon: Optional[int] = None,
                         neighbor_mask: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``nastar_soft_fields_backward`` as it is: the maps, ``tau``, ``horizon`` and mask of the ``soft_fields_forward(..., tape=True)`` call
    that wrote ``tape``, and an upstream gradient of ``dists``' shape -> ``(grad_cost [B,H,W], status [B] int32)``.  One launch on the
    current stream, nothing is read back.  ``grad_dists`` is read on the cells live at the horizon only (passable, no goal, finite
    ``dists``); ``grad_cost`` is exactly 0 on a cell that was never live.  What the backward of ``soft_cost_to_go(...,
    differentiable=True)`` runs."""
    return _soft_backward(False, False, cost_maps, goal_maps, obstacles_maps, tape, grad_dists, None, tau, horizon, neighbor_mask)


def soft_cost_to_go(cost_maps: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor, tau: float, horizon: Optional[int] = None,
                    neighbor_mask: Optional[int] = None, policies: bool = False, differentiable: bool = False) -> SoftFieldOutput:
    """The entropy-regularised (soft-min) cost-to-go field of every map of the batch over a finite horizon (include/nastar_soft_fields.h)
    -> ``SoftFieldOutput``: V_k(n) = cost[n] + softmin_tau over the allowed moves n -> m of V_{k-1}(m), ``horizon`` sweeps from "0 on the
    goals, +inf elsewhere" -- minus tau times the log of the sum of exp(-cost / tau) over the routes that reach a goal within ``horizon``
    moves.  The value function of maximum-entropy inverse RL; as ``tau`` goes to 0 it is ``cost_to_go``.  Defined for every cost >= 0
    (zero costs too), every ``tau`` > 0 and every ``horizon`` >= 1; exactly ``horizon`` sweeps run.

    ``cost_maps``, ``goal_maps``, ``obstacles_maps``: [B,1,H,W] (or [B,H,W]) float32 on one HIP device, maps of at most
    ``SOFT_FIELDS_MAX_CELLS`` cells (NotImplementedError above); a move costs the cell being left; every non-zero cell of a goal map is a
    goal.  ``tau``: a Python float, the temperature (no gradient).  ``horizon``: None = 2 * (H + W).  ``neighbor_mask``: the move set as
    the search takes it (None = Moore-8).  ``policies=True`` also returns the soft policy of the last sweep (detached).  One launch on the
    current stream; the per-map status is read before returning (one host synchronisation; not inside a stream capture): a NaN or a
    negative cost on a passable cell raises ValueError naming the rows; a map without a goal is reported in ``status``.

    ``differentiable=True``: maps of at most ``SOFT_FIELDS_GRAD_MAX_CELLS`` cells (NotImplementedError above, before anything is
    launched); the same launch also writes its tape (B * horizon * H * W fp32), and ``dists`` carries an autograd node when ``cost_maps``
    requires a gradient and grad mode is on.  Its backward is ONE launch of ``nastar_soft_fields_backward`` on the current stream and
    reads nothing back; the gradient goes to ``cost_maps`` alone and is smooth in the costs: for ``dists[b, 0, y, x]`` it is the expected
    number of visits of the soft policy on its way from (y, x) to a goal.  ``dists`` holds +inf where no goal lies within ``horizon``
    moves: a loss masks those cells itself; whatever gradient arrives for them, for goals and for obstacles is ignored."""
    return _soft_cost_to_go(False, cost_maps, goal_maps, obstacles_maps, tau, horizon, neighbor_mask, policies, differentiable)


def _soft_call(tiled: bool, what: str, cost_maps, goal_maps, obstacles_maps, tau, horizon, neighbor_mask, checkpoint_every):
    """what ``soft_cost_to_go``, ``soft_policy`` and their tiled siblings refuse before anything else, in their one order -> (B, H, W) and the
    checked ``(tau, horizon, mask, checkpoint_every)`` every raw call of the variant then takes (``checkpoint_every``: None unless tiled)"""
    _, mask, (B, H, W) = _field_inputs(cost_maps, goal_maps, obstacles_maps, neighbor_mask)
    t, K = _checked_tau(tau), _checked_horizon(horizon, H, W)
    c = None
    if tiled:
        c = _checked_checkpoint_every(checkpoint_every, K)
        _soft_tiled_limit(H, W, what)
    return (B, H, W), (t, K, mask, c)


def _soft_cost_to_go(tiled: bool, cost_maps, goal_maps, obstacles_maps, tau, horizon, neighbor_mask, policies, differentiable,
                     checkpoint_every=None) -> SoftFieldOutput:
    """the body of ``soft_cost_to_go`` and ``soft_cost_to_go_tiled``"""
    what = "soft_cost_to_go_tiled" if tiled else "soft_cost_to_go"
    (B, H, W), call = _soft_call(tiled, what, cost_maps, goal_maps, obstacles_maps, tau, horizon, neighbor_mask, checkpoint_every)
    if not tiled and differentiable and H * W > SOFT_FIELDS_GRAD_MAX_CELLS:
        raise NotImplementedError(f"soft_cost_to_go: differentiable=True takes maps of at most {SOFT_FIELDS_GRAD_MAX_CELLS} cells, got {H}x{W} = "
                                  f"{H * W} (larger maps: soft_cost_to_go_tiled(..., differentiable=True))")
    want_tape = differentiable and cost_maps.requires_grad and torch.is_grad_enabled()  # (asked here: inside the node grad mode is off)
    t, K, mask, c = call

    def field(cm, g, o):  # -> (output, tape): the node saves the tape and the costs it was made from (_FieldNode, ``taped``)
        dists, _, pol, status, tape = _soft_forward(tiled, False, cm, g, o, t, K, mask, policies, want_tape, c)
        if not torch.cuda.is_current_stream_capturing():
            _raise_bad_cost(status.cpu(), B, what)
        return SoftFieldOutput(dists, pol, status), tape

    if not differentiable:
        return field(cost_maps, goal_maps, obstacles_maps)[0]
    return SoftFieldOutput(*_differentiable_field(cost_maps, goal_maps, obstacles_maps, field,
                                                  lambda d, g, o, cm, tape, up: _soft_backward(tiled, False, cm, g, o, tape, up, None, *call)[0],
                                                  taped=True))


def maxent_path_nll(cost_maps: torch.Tensor, start_maps: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor,
                    opt_trajs: torch.Tensor, tau: float, horizon: Optional[int] = None, neighbor_mask: Optional[int] = None) -> torch.Tensor:
    """The negative log-likelihood of a demonstration under the maximum-entropy route distribution of ``cost_maps`` -> [B]:
    ``(sum of cost * opt_trajs * (1 - goal) - V_K(start)) / tau`` with V_K the field of ``soft_cost_to_go(..., differentiable=True)`` --
    the demonstration pays every cell it leaves, and exp(-V_K(start) / tau) is the partition function over the routes from the start that
    reach a goal within ``horizon`` moves, so the value is >= 0 for a demonstration among them.  Composed in torch on top of that node: the
    gradient with respect to ``cost_maps`` is (demonstration - expected visits) / tau.  ``start_maps`` is one-hot, ``opt_trajs`` the 0/1
    mask of the demonstrated route (start and goal included), both of the maps' shape.  Reads the field at the starts once (a host
    synchronisation): a start whose V_K is +inf -- no goal within ``horizon`` moves, or none at all -- raises ValueError naming the maps."""
    out = soft_cost_to_go(cost_maps, goal_maps, obstacles_maps, tau, horizon, neighbor_mask, policies=False, differentiable=True)
    return _nll_of_field(out, cost_maps, start_maps, goal_maps, opt_trajs, tau, horizon)


def _nll_of_field(out: SoftFieldOutput, cost_maps, start_maps, goal_maps, opt_trajs, tau, horizon) -> torch.Tensor:
    """what ``maxent_path_nll`` and ``maxent_path_nll_tiled`` compose on top of their field node"""
    B, _, H, W = out.dists.shape
    for name, m in (("start_maps", start_maps), ("opt_trajs", opt_trajs)):
        if not torch.is_tensor(m) or m.ndim not in (3, 4) or (m.shape[0],) + tuple(m.shape[-2:]) != (B, H, W) or m.device != out.dists.device:
            raise ValueError(f"{name} must be a [B,1,H,W] or [B,H,W] tensor of {B} maps of {H}x{W} on {out.dists.device}")
    at_start = torch.where(_maps3(start_maps) != 0, out.dists[:, 0], torch.zeros_like(out.dists[:, 0])).sum((1, 2))
    lost = torch.nonzero(~torch.isfinite(at_start.detach())).flatten().tolist()
    if lost:
        raise ValueError(f"maxent_path_nll: no goal within horizon = {_checked_horizon(horizon, H, W)} moves of the start of map(s) {lost[:16]}"
                         f"{' ...' if len(lost) > 16 else ''} ({len(lost)} of {B}): the soft cost-to-go there is +inf (a longer horizon, or an "
                         "unreachable goal)")
    leaves = _maps3(opt_trajs).to(torch.float32) * (_maps3(goal_maps) == 0).to(torch.float32)
    demo = (_maps3(cost_maps) * leaves).sum((1, 2))
    return (demo - at_start) / _checked_tau(tau)


# ---- include/nastar_soft_fields_tiled.h: the same field and gradient by tiled sweeps, with a checkpointed tape
SOFT_FIELDS_TILED_MAX_CELLS = 1179648  # nastar_soft_fields_tiled_max_cells(): 1024 x 1152, every map size the search takes


def _checked_checkpoint_every(checkpoint_every, K: int) -> int:
    if checkpoint_every is None:
        return max(1, math.isqrt(K - 1) + 1)  # ceil(sqrt(K)): about 2 sqrt(K) planes per map instead of K, for one more forward
    if isinstance(checkpoint_every, bool) or not isinstance(checkpoint_every, int) or not 1 <= checkpoint_every < 2 ** 31:
        raise ValueError(f"checkpoint_every must be a positive int or None (= ceil(sqrt(horizon))), got {checkpoint_every!r}")
    return checkpoint_every


def _soft_tiled_limit(H: int, W: int, what: str) -> None:
    if H * W > SOFT_FIELDS_TILED_MAX_CELLS:
        raise NotImplementedError(f"{what}: maps of {H}x{W} = {H * W} cells exceed the limit of {SOFT_FIELDS_TILED_MAX_CELLS} cells")


def soft_fields_tiled_forward(cost_maps: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor, tau: float,
                              horizon: Optional[int] = None, neighbor_mask: Optional[int] = None, policies: bool = False, tape: bool = False,
                              checkpoint_every: Optional[int] = None, sweeps_per_launch: Optional[int] = None):
    """``nastar_soft_cost_to_go_tiled`` as it is (include/nastar_soft_fields_tiled.h) -> ``(SoftFieldOutput, tape)``: one prepare launch and
    ceil(horizon / S) sweep launches on the current stream, nothing is read back, detached outputs.  ``tape=True`` allocates the tape of
    ``nastar_soft_fields_tiled_tape_bytes`` bytes (the planes at the multiples of ``checkpoint_every`` and plane K; None = ceil(sqrt(K)))
    and returns it as a uint8 tensor; None otherwise.  ``sweeps_per_launch``: 1 .. S instead of S, the same bits in more launches (probes
    and tests only).  What ``soft_cost_to_go_tiled`` runs."""
    dists, _, pol, status, buf = _soft_forward(True, False, cost_maps, goal_maps, obstacles_maps, tau, horizon, neighbor_mask, policies, tape,
                                               checkpoint_every, sweeps_per_launch)
    return SoftFieldOutput(dists, pol, status), buf


def soft_fields_tiled_backward(cost_maps: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor, tape: torch.Tensor,
                               grad_dists: torch.Tensor, tau: float, horizon: Optional[int] = None, neighbor_mask: Optional[int] = None,
                               checkpoint_every: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``nastar_soft_fields_backward_tiled`` as it is: the maps, ``tau``, ``horizon``, mask and ``checkpoint_every`` of the
    ``soft_fields_tiled_forward(..., tape=True)`` call that wrote ``tape``, and an upstream gradient of ``dists``' shape ->
    ``(grad_cost [B,H,W], status [B] int32)``.  One launch per step and the recomputation of every segment on the current stream, nothing
    is read back.  ``grad_dists`` is read on the cells live at the horizon only; ``grad_cost`` is exactly 0 on a cell that was never
    live.  What the backward of ``soft_cost_to_go_tiled(..., differentiable=True)`` runs."""
    return _soft_backward(True, False, cost_maps, goal_maps, obstacles_maps, tape, grad_dists, None, tau, horizon, neighbor_mask, checkpoint_every)


def soft_cost_to_go_tiled(cost_maps: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor, tau: float,
                          horizon: Optional[int] = None, neighbor_mask: Optional[int] = None, policies: bool = False,
                          differentiable: bool = False, checkpoint_every: Optional[int] = None) -> SoftFieldOutput:
    """``soft_cost_to_go`` for maps of up to ``SOFT_FIELDS_TILED_MAX_CELLS`` cells (1024x1152: every map size the search takes), by tiled
    sweeps (include/nastar_soft_fields_tiled.h) -> ``SoftFieldOutput``.  The same definition and, on the maps both take, the same bits in
    ``dists``, ``policies``, ``status`` and the gradient; the planes live in device memory, a launch runs several sweeps on every tile of
    every map, and ceil(horizon / S) + 1 launches are enqueued on the current stream.  The per-map status is read before returning as
    ``soft_cost_to_go`` reads it (not inside a stream capture), with the same ValueError for a NaN or a negative cost.

    ``differentiable=True``: the launches also keep a CHECKPOINTED tape -- the planes at the multiples of ``checkpoint_every`` and the
    last one -- and ``dists`` carries an autograd node when ``cost_maps`` requires a gradient and grad mode is on.  The backward rebuilds
    each segment of planes from its checkpoint (the forward is a pure function: the same bits) and walks it back, one launch per step,
    reading nothing back.  ``checkpoint_every=None`` is ceil(sqrt(horizon)): about 2 sqrt(horizon) planes per map instead of ``horizon``,
    for one more forward; ``checkpoint_every=1`` keeps every plane, for the caller who has the memory.  The gradient does not depend on
    it."""
    return _soft_cost_to_go(True, cost_maps, goal_maps, obstacles_maps, tau, horizon, neighbor_mask, policies, differentiable, checkpoint_every)


def maxent_path_nll_tiled(cost_maps: torch.Tensor, start_maps: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor,
                          opt_trajs: torch.Tensor, tau: float, horizon: Optional[int] = None, neighbor_mask: Optional[int] = None,
                          checkpoint_every: Optional[int] = None) -> torch.Tensor:
    """``maxent_path_nll`` composed on ``soft_cost_to_go_tiled(..., differentiable=True, checkpoint_every=checkpoint_every)``: the same
    loss and gradient for maps of up to ``SOFT_FIELDS_TILED_MAX_CELLS`` cells.  What the planners' ``maxent_path_nll(..., tiled=True)``
    calls."""
    out = soft_cost_to_go_tiled(cost_maps, goal_maps, obstacles_maps, tau, horizon, neighbor_mask, policies=False, differentiable=True,
                                checkpoint_every=checkpoint_every)
    return _nll_of_field(out, cost_maps, start_maps, goal_maps, opt_trajs, tau, horizon)


# ---- include/nastar_soft_policy.h: the log-policy of the soft field and the gradient through it ---------------
class SoftPolicyOutput(NamedTuple):
    """What ``soft_policy()`` returns.  ``dists`` [B,1,H,W] fp32: the field of ``soft_cost_to_go``; ``log_policies`` [B,8,H,W] fp32: the log
    of the soft policy of the last sweep (action k = ``utils.synthetic.ACTION_MOVES[k]``), -inf for a move the mask, the border or an
    obstacle forbids or whose target has no goal within ``horizon`` - 1 moves, and for all eight actions of a goal, an obstacle and a cell
    with an infinite ``dists``; ``policies`` [B,8,H,W] fp32: that policy itself, detached (0 where the log is -inf), or None; ``status``
    [B] int32 as in ``SoftFieldOutput``."""

    dists: torch.Tensor
    log_policies: torch.Tensor
    policies: Optional[torch.Tensor]
    status: torch.Tensor


def soft_policy_forward(cost_maps: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor, tau: float, horizon: Optional[int] = None,
                        neighbor_mask: Optional[int] = None, policies: bool = True, tape: bool = False):
    """``nastar_soft_policy_forward`` as it is (include/nastar_soft_policy.h) -> ``(SoftPolicyOutput, tape)``: ``soft_fields_forward`` with
    the log-policy beside its outputs -- one launch on the current stream, nothing is read back, detached outputs, the same bits in
    ``dists``, ``policies``, ``status`` and the tape.  What ``soft_policy`` runs; probes and tests call it directly."""
    out = _soft_forward(False, True, cost_maps, goal_maps, obstacles_maps, tau, horizon, neighbor_mask, policies, tape)
    return SoftPolicyOutput(*out[:4]), out[4]


def soft_policy_backward(cost_maps: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor, tape: torch.Tensor,
                         grad_dists: Optional[torch.Tensor], grad_log_policies: Optional[torch.Tensor], tau: float,
                         horizon: Optional[int] = None, neighbor_mask: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``nastar_soft_policy_backward`` as it is: the maps, ``tau``, ``horizon`` and mask of the forward that wrote ``tape``
    (``soft_policy_forward`` or ``soft_fields_forward``, ``tape=True``), an upstream gradient of ``dists`` and one of ``log_policies``
    ([B,8,H,W]); either may be None (zeros) -> ``(grad_cost [B,H,W], status [B] int32)``.  One launch on the current stream, nothing is read
    back.  ``grad_log_policies`` is read only where the log-policy is finite; with None for it the result is ``soft_fields_backward``'s, bit
    for bit.  What the backward of ``soft_policy`` runs."""
    return _soft_backward(False, True, cost_maps, goal_maps, obstacles_maps, tape, grad_dists, grad_log_policies, tau, horizon, neighbor_mask)


def _soft_policy_checked(tiled: bool, cost_maps, goal_maps, obstacles_maps, call, tape: bool):
    """the raw forward of ``soft_policy`` / ``soft_policy_tiled`` (``call``: ``_soft_call``'s) and their one status read (none inside a stream
    capture) -> ``(dists, log_policies, policies, status, tape or None)``"""
    t, K, mask, c = call
    out = _soft_forward(tiled, True, cost_maps, goal_maps, obstacles_maps, t, K, mask, True, tape, c)
    if not torch.cuda.is_current_stream_capturing():
        _raise_bad_cost(out[3].cpu(), out[3].numel(), "soft_policy_tiled" if tiled else "soft_policy")
    return out


class _SoftPolicyNode(torch.autograd.Function):
    """``soft_policy_forward`` -- ``tiled``: ``soft_policy_tiled_forward`` -- as ONE autograd node with two differentiable outputs, ``dists``
    and ``log_policies``: its backward is one call of ``nastar_soft_policy_backward`` (``nastar_soft_policy_backward_tiled``) with whichever
    of the two upstream gradients arrived, and reads nothing back.  ``call``: the checked ``(tau, horizon, mask, checkpoint_every)``."""

    @staticmethod
    def forward(ctx, cost_maps, goal_maps, obstacles_maps, tiled, call):
        dists, log_policies, policies, status, tape = _soft_policy_checked(tiled, cost_maps, goal_maps, obstacles_maps, call, tape=True)
        ctx.save_for_backward(cost_maps, goal_maps, obstacles_maps, tape)
        ctx.tiled, ctx.call = tiled, call
        ctx.mark_non_differentiable(policies, status)
        ctx.set_materialize_grads(False)
        return dists, log_policies, policies, status

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_dists, g_logp, *unused):
        if (g_dists is None and g_logp is None) or not ctx.needs_input_grad[0]:
            return (None,) * 5
        cost_maps, goal_maps, obstacles_maps, tape = ctx.saved_tensors
        grad = _soft_backward(ctx.tiled, True, cost_maps, goal_maps, obstacles_maps, tape, g_dists, g_logp, *ctx.call)[0]
        return (_widen_grad(grad, tuple(cost_maps.shape)), None, None, None, None)


def _soft_policy(tiled: bool, cost_maps, goal_maps, obstacles_maps, tau, horizon, neighbor_mask, checkpoint_every=None) -> SoftPolicyOutput:
    """the body of ``soft_policy`` and ``soft_policy_tiled``"""
    what = "soft_policy_tiled" if tiled else "soft_policy"
    (B, H, W), call = _soft_call(tiled, what, cost_maps, goal_maps, obstacles_maps, tau, horizon, neighbor_mask, checkpoint_every)
    if cost_maps.requires_grad and torch.is_grad_enabled():
        if not tiled and H * W > SOFT_FIELDS_GRAD_MAX_CELLS:
            raise NotImplementedError(f"soft_policy: a differentiable call takes maps of at most {SOFT_FIELDS_GRAD_MAX_CELLS} cells, got {H}x{W} = "
                                      f"{H * W}")
        return SoftPolicyOutput(*_SoftPolicyNode.apply(cost_maps, goal_maps, obstacles_maps, tiled, call))
    return SoftPolicyOutput(*_soft_policy_checked(tiled, cost_maps, goal_maps, obstacles_maps, call, tape=False)[:4])


def soft_policy(cost_maps: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor, tau: float, horizon: Optional[int] = None,
                neighbor_mask: Optional[int] = None) -> SoftPolicyOutput:
    """The soft field of ``soft_cost_to_go`` together with the LOG of its soft policy, both differentiable (include/nastar_soft_policy.h)
    -> ``SoftPolicyOutput``: ``log_policies[b, a, y, x]`` = -(V_{K-1}(target of a) - min) / tau - ln(S) with min and S the soft-min's
    minimum and sum at (y, x), formed inside the kernel from the two kept apart -- finite where ``log(policies)`` has underflowed to -inf,
    and free of the rounding of |V| that a log-probability rebuilt from ``dists`` carries.  The arguments are those of
    ``soft_cost_to_go``; ``tau`` has no gradient.

    When ``cost_maps`` requires a gradient and grad mode is on, ``dists`` and ``log_policies`` are the two outputs of ONE autograd node
    (maps of at most ``SOFT_FIELDS_GRAD_MAX_CELLS`` cells, NotImplementedError above, before anything is launched; the launch also
    writes the tape of ``soft_cost_to_go``): its backward is one launch on the current stream and reads nothing back.  The gradient of
    ``log_policies`` is read only where they are finite, so a loss may leave anything -- a NaN too -- on the -inf entries' gradient; it
    masks the -inf VALUES itself (``torch.where``, not a product).  Otherwise no graph is built and maps of up to
    ``SOFT_FIELDS_MAX_CELLS`` cells are taken.  ``policies`` is detached either way.  The per-map status is read before returning as
    ``soft_cost_to_go`` reads it (one host synchronisation; not inside a stream capture), with the same ValueError for a NaN or a
    negative cost."""
    return _soft_policy(False, cost_maps, goal_maps, obstacles_maps, tau, horizon, neighbor_mask)


def soft_policy_nll(cost_maps: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor, opt_policies: torch.Tensor, tau: float,
                    horizon: Optional[int] = None, neighbor_mask: Optional[int] = None) -> torch.Tensor:
    """The per-cell imitation loss of the soft policy of ``cost_maps`` against the demonstrated actions ``opt_policies`` -> [B]: per map the
    mean over the counted cells of ``-sum over a of opt_policies[a, n] * log_policies[a, n]``, the cross-entropy the planning datasets'
    ``opt_policies`` were made for.  ``opt_policies`` is [B,8,H,W] in the action order of ``policies`` / ``FieldOutput.policies`` / the
    dataset (one-hot, or any non-negative weights).  A cell is counted when it is live at the horizon (passable, no goal, a finite
    ``dists``) and its ``opt_policies`` row is not all zero; a map with no counted cell gives 0.  Composed in torch on the node of
    ``soft_policy``: the gradient goes to ``cost_maps``.  Reads one flag back (a host synchronisation): a counted cell whose demonstrated
    action has a log-probability of -inf -- a move the mask or an obstacle forbids, or onto a cell with no goal within ``horizon`` - 1
    moves -- raises ValueError naming the maps."""
    _check_opt_policies(cost_maps, goal_maps, obstacles_maps, opt_policies, neighbor_mask)
    out = soft_policy(cost_maps, goal_maps, obstacles_maps, tau, horizon, neighbor_mask)
    return _nll_of_policy(out, opt_policies, horizon)


def _check_opt_policies(cost_maps, goal_maps, obstacles_maps, opt_policies, neighbor_mask) -> None:
    _, _, (B, H, W) = _field_inputs(cost_maps, goal_maps, obstacles_maps, neighbor_mask)
    if not torch.is_tensor(opt_policies) or tuple(opt_policies.shape) != (B, 8, H, W) or opt_policies.device != cost_maps.device:
        raise ValueError(f"opt_policies must be a [B,8,H,W] tensor for {B} maps of {H}x{W} on {cost_maps.device}, got "
                         f"{(tuple(opt_policies.shape), str(opt_policies.device)) if torch.is_tensor(opt_policies) else type(opt_policies).__name__}")


def _nll_of_policy(out: SoftPolicyOutput, opt_policies: torch.Tensor, horizon) -> torch.Tensor:
    """what ``soft_policy_nll`` and ``soft_policy_nll_tiled`` compose on top of their policy node"""
    B, _, H, W = out.dists.shape
    logp = out.log_policies
    weights = opt_policies.to(torch.float32)
    shown = weights != 0
    counted = torch.isfinite(logp.detach()).any(1) & shown.any(1)        # live at the horizon: some action has a finite log-probability
    pick = shown & counted[:, None]
    lost = torch.nonzero((pick & torch.isinf(logp.detach())).flatten(1).any(1)).flatten().tolist()
    if lost:
        raise ValueError(f"soft_policy_nll: a demonstrated action of map(s) {lost[:16]}{' ...' if len(lost) > 16 else ''} ({len(lost)} of {B}) has "
                         f"probability 0 under the soft policy: the move is outside the mask or onto an obstacle, or its target has no goal within "
                         f"horizon - 1 = {_checked_horizon(horizon, H, W) - 1} moves")
    terms = weights * torch.where(pick, logp, torch.zeros_like(logp))     # (where, not a product: no 0 * -inf)
    return -terms.sum((1, 2, 3)) / counted.sum((1, 2)).clamp(min=1).to(torch.float32)


# ---- include/nastar_soft_policy_tiled.h: the log-policy and its gradient by tiled sweeps, with the checkpointed tape
def soft_policy_tiled_forward(cost_maps: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor, tau: float,
                              horizon: Optional[int] = None, neighbor_mask: Optional[int] = None, policies: bool = True, tape: bool = False,
                              checkpoint_every: Optional[int] = None, sweeps_per_launch: Optional[int] = None):
    """``nastar_soft_policy_forward_tiled`` as it is (include/nastar_soft_policy_tiled.h) -> ``(SoftPolicyOutput, tape)``:
    ``soft_fields_tiled_forward`` with the log-policy beside its outputs, written by the launch that reaches the horizon -- the same
    launches on the current stream, nothing is read back, detached outputs, the same bits in ``dists``, ``policies``, ``status`` and the
    tape.  ``tape``, ``checkpoint_every`` and ``sweeps_per_launch`` as there.  What ``soft_policy_tiled`` runs."""
    out = _soft_forward(True, True, cost_maps, goal_maps, obstacles_maps, tau, horizon, neighbor_mask, policies, tape, checkpoint_every,
                        sweeps_per_launch)
    return SoftPolicyOutput(*out[:4]), out[4]


def soft_policy_tiled_backward(cost_maps: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor, tape: torch.Tensor,
                               grad_dists: Optional[torch.Tensor], grad_log_policies: Optional[torch.Tensor], tau: float,
                               horizon: Optional[int] = None, neighbor_mask: Optional[int] = None,
                               checkpoint_every: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``nastar_soft_policy_backward_tiled`` as it is: the maps, ``tau``, ``horizon``, mask and ``checkpoint_every`` of the tiled forward
    that wrote ``tape`` (``soft_policy_tiled_forward`` or ``soft_fields_tiled_forward``, ``tape=True``), an upstream gradient of ``dists``
    and one of ``log_policies`` ([B,8,H,W]); either may be None (zeros) -> ``(grad_cost [B,H,W], status [B] int32)``.  The launches of
    ``soft_fields_tiled_backward`` on the current stream, the one of step ``horizon`` carrying the log-policy seed; nothing is read back.
    ``grad_log_policies`` is read only where the log-policy is finite; with None for it the result is ``soft_fields_tiled_backward``'s,
    bit for bit.  What the backward of ``soft_policy_tiled`` runs."""
    return _soft_backward(True, True, cost_maps, goal_maps, obstacles_maps, tape, grad_dists, grad_log_policies, tau, horizon, neighbor_mask,
                          checkpoint_every)


def soft_policy_tiled(cost_maps: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor, tau: float, horizon: Optional[int] = None,
                      neighbor_mask: Optional[int] = None, checkpoint_every: Optional[int] = None) -> SoftPolicyOutput:
    """``soft_policy`` for maps of up to ``SOFT_FIELDS_TILED_MAX_CELLS`` cells (1024x1152: every map size the search takes), by tiled sweeps
    (include/nastar_soft_policy_tiled.h) -> ``SoftPolicyOutput``.  The same definition and, on the maps both take, the same bits in
    ``dists``, ``log_policies``, ``policies``, ``status`` and the gradient; NotImplementedError above the limit, before anything is
    launched.  The log-policy is written by the sweep launch that reaches the horizon: the launches are those of
    ``soft_cost_to_go_tiled``.

    When ``cost_maps`` requires a gradient and grad mode is on, ``dists`` and ``log_policies`` are the two outputs of ONE autograd node
    that keeps the CHECKPOINTED tape of ``soft_cost_to_go_tiled`` (``checkpoint_every``: None = ceil(sqrt(horizon)), 1 keeps every plane;
    the gradient does not depend on it).  Its backward is that call's backward, one launch per step, with the launch of step ``horizon``
    carrying the gradient of ``log_policies``; it reads nothing back.  The gradient of ``log_policies`` is read only where they are
    finite.  Otherwise no graph is built and no tape is kept.  ``policies`` is detached either way.  The per-map status is read once
    before returning (not inside a stream capture), with the ValueError of ``soft_policy`` for a NaN or a negative cost."""
    return _soft_policy(True, cost_maps, goal_maps, obstacles_maps, tau, horizon, neighbor_mask, checkpoint_every)


def soft_policy_nll_tiled(cost_maps: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor, opt_policies: torch.Tensor, tau: float,
                          horizon: Optional[int] = None, neighbor_mask: Optional[int] = None,
                          checkpoint_every: Optional[int] = None) -> torch.Tensor:
    """``soft_policy_nll`` composed on ``soft_policy_tiled(..., checkpoint_every=checkpoint_every)``: the same loss and gradient for maps of
    up to ``SOFT_FIELDS_TILED_MAX_CELLS`` cells -- the size ``cost_to_go_tiled`` builds ``opt_policies`` for.  What the planners'
    ``policy_nll(..., tiled=True)`` calls."""
    _check_opt_policies(cost_maps, goal_maps, obstacles_maps, opt_policies, neighbor_mask)
    out = soft_policy_tiled(cost_maps, goal_maps, obstacles_maps, tau, horizon, neighbor_mask, checkpoint_every)
    return _nll_of_policy(out, opt_policies, horizon)


# ---- include/nastar_soft_routes.h: sampled routes from the maximum-entropy route distribution of the soft field
SOFT_ROUTES_MAX_CELLS = 12288  # nastar_soft_routes_max_cells(): every size the one-workgroup forward takes -- it writes a tape at each
SOFT_ROUTES_MAX_WALKERS = 1 << 30  # the most (map, start, sample) walkers one call takes
SOFT_ROUTES_SHAPES = {None: 0, "lds": 1, "gather": 2}  # ``shape`` of soft_routes_from_tape: the library's choice, or one kernel shape


class SoftRoutes(NamedTuple):
    """What ``soft_routes()`` returns: N sampled routes per (map, start) query.  ``routes`` [B,S,N,L] int32: flat cell indices r*W + c in
    travel order, the goal last, then -1; a route longer than L keeps its LAST L cells.  ``route_lengths`` [B,S,N] int32: the true number of
    route cells (at most horizon + 1).  ``route_costs`` [B,S,N] fp32: the cost of every route cell but the last.  ``log_probs`` [B,S,N]
    fp32: log p(route) under the maximum-entropy route distribution, ``(dists[start] - route_costs) / tau`` up to rounding.  ``visits``
    [B,S,H,W] int32 or None: how often the N routes of a query stood on each cell, the final goal cell not counted.  ``dists`` [B,1,H,W]:
    the soft field V_K the walk was drawn from.  ``status`` [B,S] int32: 0, 1 (the index lies outside [0, H*W)), ``FIELD_BAD_COST`` (9) or
    ``STATUS_UNSOLVABLE`` (3: ``dists`` is not finite at the start); a failed query has lengths 0, rows of -1, costs +inf and log_probs
    -inf.  ``map_status`` [B] int32: the forward's per-map status."""

    routes: torch.Tensor
    route_lengths: torch.Tensor
    route_costs: torch.Tensor
    log_probs: torch.Tensor
    visits: Optional[torch.Tensor]
    dists: torch.Tensor
    status: torch.Tensor
    map_status: torch.Tensor


def _checked_samples(num_samples) -> int:
    if isinstance(num_samples, bool) or not isinstance(num_samples, int) or num_samples < 1:
        raise ValueError(f"num_samples must be an int >= 1, got {num_samples!r}")
    return num_samples


def _checked_seed(seed) -> int:
    """``seed`` of the samplers: an int that fits the C call's long long, or None = one 63-bit draw from torch's default CPU generator"""
    if seed is None:
        return int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
    if isinstance(seed, bool) or not isinstance(seed, int) or not -2 ** 63 <= seed < 2 ** 63:
        raise ValueError(f"seed must be an int in [-2**63, 2**63) or None (drawn from torch's default generator), got {seed!r}")
    return seed


def _checked_sample_len(max_route_len) -> None:
    if max_route_len is not None and (isinstance(max_route_len, bool) or not isinstance(max_route_len, int) or max_route_len < 1):
        raise ValueError(f"max_route_len must be an int >= 1 (or None: horizon + 1, which no route outgrows), got {max_route_len!r}")


def _soft_routes_limit(tiled: bool, H: int, W: int) -> None:
    if tiled:
        _soft_tiled_limit(H, W, "soft_routes_tiled")
    elif H * W > SOFT_ROUTES_MAX_CELLS:
        raise NotImplementedError(f"soft_routes: maps of {H}x{W} = {H * W} cells exceed the limit of {SOFT_ROUTES_MAX_CELLS} cells (the "
                                  "one-workgroup soft field; larger maps: soft_routes_tiled)")


def _soft_routes_from_tape(tiled: bool, cost_maps, goal_maps, obstacles_maps, tape, starts, tau, horizon, num_samples, seed, neighbor_mask,
                           max_route_len, visits, uniforms, shape=None, checkpoint_every=None):
    """the raw walker call of ``soft_routes_from_tape`` and ``soft_routes_tiled_from_tape``: the refusals in one order, the outputs, ONE C
    call with its arguments in header order -> ``(routes, route_lengths, route_costs, log_probs, visits or None, status)``.  ``tiled``:
    ``checkpoint_every`` and a workspace, which the one-workgroup call does not have; ``shape`` is the one-workgroup call's."""
    what = "soft_routes_tiled" if tiled else "soft_routes"
    t = _checked_tau(tau)
    maps, mask, (B, H, W) = _field_inputs(cost_maps, goal_maps, obstacles_maps, neighbor_mask)
    K = _checked_horizon(horizon, H, W)
    N = _checked_samples(num_samples)
    seed = _checked_seed(seed)
    _checked_sample_len(max_route_len)
    if tiled:
        c = _checked_checkpoint_every(checkpoint_every, K)
    elif shape not in SOFT_ROUTES_SHAPES:
        raise ValueError(f"shape must be None, 'lds' or 'gather', got {shape!r}")
    _soft_routes_limit(tiled, H, W)
    idx = _start_indices(starts, B, H, W)
    S = idx.shape[1]
    if B * S * N > SOFT_ROUTES_MAX_WALKERS:
        raise NotImplementedError(f"{what}: {B} maps x {S} starts x {N} samples exceed the limit of {SOFT_ROUTES_MAX_WALKERS} walkers per call")
    if uniforms is not None and (not torch.is_tensor(uniforms) or uniforms.dtype != torch.float32 or tuple(uniforms.shape) != (B, S, N, K)):
        raise ValueError(f"uniforms must be a float32 tensor of shape ({B}, {S}, {N}, {K}) = [B,S,N,horizon], got "
                         f"{tuple(uniforms.shape) if torch.is_tensor(uniforms) else type(uniforms).__name__}")
    dev = _field_device(maps)
    for name, x in (("starts", idx), ("uniforms", uniforms)):
        if x is not None and x.device != dev:
            raise ValueError(f"the maps live on {dev}, {name} on {x.device}: they must share a device")
    symbol = "nastar_soft_routes_tiled" if tiled else "nastar_soft_routes"
    lib = _field_lib(symbol, symbol + ".h")
    if not torch.is_tensor(tape) or tape.dtype != torch.uint8 or tape.device != dev or not tape.is_contiguous():
        raise ValueError(f"tape must be the contiguous uint8 tensor soft_fields{'_tiled' if tiled else ''}_forward(..., tape=True) returned, on {dev}")
    cap = K + 1 if max_route_len is None else max_route_len
    with torch.no_grad():
        cost, goal, passable = (_maps3(m.detach()) for m in maps)
        idx = idx.contiguous()
        uni = None if uniforms is None else uniforms.detach().contiguous()
        routes = torch.empty((B, S, N, cap), dtype=torch.int32, device=dev)
        lengths = torch.empty((B, S, N), dtype=torch.int32, device=dev)
        costs = torch.empty((B, S, N), dtype=torch.float32, device=dev)
        logp = torch.empty((B, S, N), dtype=torch.float32, device=dev)
        counts = torch.empty((B, S, H, W), dtype=torch.int32, device=dev) if visits else None
        status = torch.empty((B, S), dtype=torch.int32, device=dev)
        args = (cost.data_ptr(), goal.data_ptr(), passable.data_ptr(), tape.data_ptr(), tape.numel()) + ((c,) if tiled else ())
        args += (idx.data_ptr(), B, S, N, H, W, mask, t, K, seed, _ptr(uni), routes.data_ptr(), cap, lengths.data_ptr(), costs.data_ptr(),
                 logp.data_ptr(), _ptr(counts), status.data_ptr())
        entry = symbol
        if tiled:
            ws_bytes = int(lib.nastar_soft_routes_tiled_workspace_bytes(B, S, N, H, W, K, c))
            ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
            args += (ws.data_ptr(), ws_bytes)
        elif shape is not None:
            entry, args = symbol + "_with_shape", args + (SOFT_ROUTES_SHAPES[shape],)
        with torch.cuda.device(dev):
            rc = getattr(lib, entry)(*args, _stream_ptr(dev))
        _native.check(rc, symbol)
    return routes, lengths, costs, logp, counts, status


def _soft_routes(tiled: bool, cost_maps, goal_maps, obstacles_maps, starts, tau, horizon, num_samples, seed, neighbor_mask, max_route_len, visits,
                 uniforms, checkpoint_every=None, differentiable: bool = False) -> "SoftRoutes":
    """the body of ``soft_routes`` and ``soft_routes_tiled``: the refusals before anything is launched, the forward with its tape, the
    walkers; ``differentiable``: ``log_probs`` as the output of ``_SoftRoutesNode`` when there is something to differentiate"""
    N = _checked_samples(num_samples)
    _checked_sample_len(max_route_len)
    seed = _checked_seed(seed)
    if not isinstance(differentiable, bool):
        raise TypeError(f"differentiable must be a bool, got {differentiable!r}")
    _, _, (B, H, W) = _field_inputs(cost_maps, goal_maps, obstacles_maps, neighbor_mask)
    _soft_routes_limit(tiled, H, W)
    idx = _start_indices(starts, B, H, W)  # (refused before the forward launches anything)
    if differentiable:
        if tiled:
            raise NotImplementedError("soft_routes_tiled: differentiable=True is not built (the score-function backward reads the whole tape of "
                                      f"the one-workgroup field: soft_routes(..., differentiable=True), maps of at most {SOFT_ROUTES_GRAD_MAX_CELLS} cells)")
        _checked_tau(tau)
        K = _checked_horizon(horizon, H, W)
        if max_route_len is not None and max_route_len < K + 1:
            raise ValueError(f"soft_routes: differentiable=True needs max_route_len >= horizon + 1 = {K + 1} (or None), got {max_route_len}: the "
                             "backward reads whole routes and does not replay walks")
        _soft_routes_grad_limits("soft_routes: differentiable=True", H, W, idx.shape[1], N, K)
        if cost_maps.requires_grad and torch.is_grad_enabled():
            return SoftRoutes(*_SoftRoutesNode.apply(cost_maps, goal_maps, obstacles_maps, idx, uniforms,
                                                     (tau, K, N, seed, neighbor_mask, max_route_len, visits)))
    return _soft_routes_run(tiled, cost_maps, goal_maps, obstacles_maps, starts, tau, horizon, num_samples, seed, neighbor_mask, max_route_len,
                            visits, uniforms, checkpoint_every)[0]


def _soft_routes_run(tiled: bool, cost_maps, goal_maps, obstacles_maps, starts, tau, horizon, num_samples, seed, neighbor_mask, max_route_len, visits,
                     uniforms, checkpoint_every=None):
    """the launches of ``_soft_routes``, its arguments checked: the forward with its tape, then the walkers -> ``(SoftRoutes, tape)``"""
    dists, _, _, map_status, tape = _soft_forward(tiled, False, cost_maps, goal_maps, obstacles_maps, tau, horizon, neighbor_mask, False, True,
                                                  checkpoint_every, tape_limit=SOFT_ROUTES_MAX_CELLS)
    routes, lengths, costs, logp, counts, status = _soft_routes_from_tape(tiled, cost_maps, goal_maps, obstacles_maps, tape, starts, tau, horizon,
                                                                          num_samples, seed, neighbor_mask, max_route_len, visits, uniforms,
                                                                          checkpoint_every=checkpoint_every)
    return SoftRoutes(routes, lengths, costs, logp, counts, dists, status, map_status), tape


def soft_routes_from_tape(cost_maps: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor, tape: torch.Tensor,
                          starts: torch.Tensor, tau: float, horizon: Optional[int] = None, num_samples: int = 1, seed: int = 0,
                          neighbor_mask: Optional[int] = None, max_route_len: Optional[int] = None, visits: bool = False,
                          uniforms: Optional[torch.Tensor] = None, shape: Optional[str] = None):
    """``nastar_soft_routes`` as it is (include/nastar_soft_routes.h) -> ``(routes, route_lengths, route_costs, log_probs, visits or None,
    status)``: the maps, ``tau``, ``horizon`` and mask of the ``soft_fields_forward(..., tape=True)`` call that wrote ``tape``.  Two
    launches (the rows' -1 and the counts' zeros, then the walkers) on the current stream, nothing is read back: it can be captured into a graph.  ``seed``: an int (the Philox key);
    ``uniforms``: a float32 [B,S,N,horizon] tensor that replaces the generator.  ``max_route_len=None``: rows of ``horizon + 1`` cells, which
    no route outgrows.  ``shape``: None, or "lds" / "gather" to pick the kernel shape (probes and tests; the same bits).  What
    ``soft_routes`` runs behind its forward."""
    return _soft_routes_from_tape(False, cost_maps, goal_maps, obstacles_maps, tape, starts, tau, horizon, num_samples, seed, neighbor_mask,
                                  max_route_len, visits, uniforms, shape)


def soft_routes(cost_maps: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor, starts: torch.Tensor, tau: float,
                horizon: Optional[int] = None, num_samples: int = 1, seed: Optional[int] = None, neighbor_mask: Optional[int] = None,
                max_route_len: Optional[int] = None, visits: bool = False, uniforms: Optional[torch.Tensor] = None,
                differentiable: bool = False) -> SoftRoutes:
    """SAMPLE routes from the maximum-entropy route distribution of ``cost_maps`` (include/nastar_soft_routes.h) -> ``SoftRoutes``:
    ``num_samples`` independent routes from each of S start cells per map, drawn with probability exp((V_K(start) - cost(route)) / tau)
    among the routes that reach a goal within ``horizon`` moves -- the distribution ``maxent_path_nll`` trains.  The walker with k moves
    left draws from pi_k, the softmax of -V_{k-1} / tau: the non-stationary chain, not the one plane ``soft_cost_to_go(policies=True)``
    returns.  As ``tau`` goes to 0 every sample is ``field_routes``' optimal route.

    The maps, ``tau``, ``horizon`` and ``neighbor_mask`` of ``soft_cost_to_go``, maps of at most ``SOFT_ROUTES_MAX_CELLS`` cells
    (NotImplementedError above; larger maps: ``soft_routes_tiled``).
    ``starts``: an integer [B,S] tensor of flat cell indices r*W + c, or a float [B,S,H,W] tensor of start maps (``field_routes``).
    ``seed``: an int, or None = one 63-bit draw from torch's default CPU generator (``torch.manual_seed`` makes a run repeatable); a sample
    is a pure function of the inputs, the seed and its (map, start, sample) numbers: the same seed gives the same bits, and the first N
    samples of a query do not change when ``num_samples`` grows.  ``uniforms``: a float32 [B,S,N,horizon] tensor of the walkers' own
    uniform numbers instead.  ``max_route_len``: the row length of ``routes`` (a longer route keeps its last cells); None = horizon + 1,
    which no route outgrows.  ``visits=True`` also counts the cells the routes stood on.

    An EVALUATION call on the current stream of the inputs' device: the forward launch with its tape (B * horizon * H * W fp32), a
    launch that clears the rows and the counts and the walkers' launch; detached outputs, nothing is read back -- it can be captured into a graph -- and nothing raises for a
    failed query or a bad map: read ``status`` and ``map_status``.

    ``differentiable=True``: the same launches and the same bits, and ``log_probs`` is the one differentiable output of an autograd node
    when ``cost_maps`` requires a gradient and grad mode is on -- the SCORE-FUNCTION estimator: the routes are samples, not functions of
    the costs, and log p(route) = (V_K(start) - cost(route)) / tau is.  Its backward is ``soft_routes_backward`` (include/
    nastar_soft_routes_grad.h): at most five launches on the current stream, nothing read back, the same bits from two calls; the gradient
    goes to ``cost_maps`` alone.  The gradient that arrives for the ``log_probs`` of a failed query is never read; ``log_probs`` is -inf
    there, so a loss masks those entries with ``torch.where`` -- ``route_score_loss`` does.  Every other output stays detached.  Refused
    before anything is launched: ``max_route_len`` below ``horizon + 1`` (ValueError: the backward reads whole routes), maps of more than
    ``SOFT_ROUTES_GRAD_MAX_CELLS`` cells and S * N * horizon above 2^31 (NotImplementedError)."""
    return _soft_routes(False, cost_maps, goal_maps, obstacles_maps, starts, tau, horizon, num_samples, seed, neighbor_mask, max_route_len, visits,
                        uniforms, differentiable=differentiable)


# ---- include/nastar_soft_routes_grad.h: the score-function backward of the sampled routes
SOFT_ROUTES_GRAD_MAX_CELLS = 6144  # nastar_soft_routes_grad_max_cells(): the limit of the field's backward
SOFT_ROUTES_GRAD_MIN_BITS = 30  # the fewest fraction bits P = min(40, 61 - ceil(log2(S * N * horizon))) a call may be left with


def _soft_routes_grad_limits(what: str, H: int, W: int, S: int, N: int, K: int) -> None:
    """what the score-function backward refuses beyond the walkers' own limits: the map size and the P rule"""
    if H * W > SOFT_ROUTES_GRAD_MAX_CELLS:
        raise NotImplementedError(f"{what}: maps of {H}x{W} = {H * W} cells exceed the limit of {SOFT_ROUTES_GRAD_MAX_CELLS} cells of the "
                                  f"backward (the forward alone takes {SOFT_ROUTES_MAX_CELLS})")
    bits = min(40, 61 - (S * N * K - 1).bit_length())
    if bits < SOFT_ROUTES_GRAD_MIN_BITS:
        raise NotImplementedError(f"{what}: {S} starts x {N} samples x horizon {K} leave {bits} fraction bits to the fixed-point sums, fewer than "
                                  f"{SOFT_ROUTES_GRAD_MIN_BITS} (S * N * horizon must stay at or below 2^31: split the samples over calls)")


def soft_routes_backward(cost_maps: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor, tape: torch.Tensor,
                         starts: torch.Tensor, routes: torch.Tensor, route_lengths: torch.Tensor, status: torch.Tensor,
                         grad_log_probs: torch.Tensor, tau: float, horizon: Optional[int] = None,
                         neighbor_mask: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``nastar_soft_routes_backward`` as it is (include/nastar_soft_routes_grad.h) -> ``(grad_cost [B,H,W], status [B] int32)``: the
    gradient with respect to the costs of ``(grad_log_probs * log_probs).sum()``.  The maps, ``tau``, ``horizon`` and mask of the
    ``soft_fields_forward(..., tape=True)`` call that wrote ``tape``; ``starts`` and the ``routes`` [B,S,N,L >= horizon + 1] int32,
    ``route_lengths`` [B,S,N] int32 and ``status`` [B,S] int32 of the walkers' call; ``grad_log_probs`` [B,S,N] float32, never read at a
    failed query.  At most five launches on the current stream, nothing is read back: it can be captured into a graph.  Fixed-point sums:
    the same bits from two calls.  What the backward of ``soft_routes(..., differentiable=True)`` runs."""
    t = _checked_tau(tau)
    maps, mask, (B, H, W) = _field_inputs(cost_maps, goal_maps, obstacles_maps, neighbor_mask)
    K = _checked_horizon(horizon, H, W)
    idx = _start_indices(starts, B, H, W)
    S = idx.shape[1]
    if not torch.is_tensor(routes) or routes.dtype != torch.int32 or routes.ndim != 4 or tuple(routes.shape[:2]) != (B, S) or routes.shape[2] < 1:
        raise ValueError(f"routes must be the int32 [B,S,N,L] tensor of soft_routes for {B} maps and {S} starts, got "
                         f"{tuple(routes.shape) if torch.is_tensor(routes) else type(routes).__name__}")
    N, cap = int(routes.shape[2]), int(routes.shape[3])
    if cap < K + 1:
        raise ValueError(f"soft_routes_backward: routes has rows of {cap} cells, fewer than horizon + 1 = {K + 1}: the backward reads whole "
                         "routes and does not replay walks")
    for name, x, dtype, shape in (("route_lengths", route_lengths, torch.int32, (B, S, N)), ("status", status, torch.int32, (B, S)),
                                  ("grad_log_probs", grad_log_probs, torch.float32, (B, S, N))):
        if not torch.is_tensor(x) or x.dtype != dtype or tuple(x.shape) != shape:
            raise ValueError(f"{name} must be a {str(dtype).replace('torch.', '')} tensor of shape {shape}, got "
                             f"{(tuple(x.shape), x.dtype) if torch.is_tensor(x) else type(x).__name__}")
    if B * S * N > SOFT_ROUTES_MAX_WALKERS:
        raise NotImplementedError(f"soft_routes_backward: {B} maps x {S} starts x {N} samples exceed the limit of {SOFT_ROUTES_MAX_WALKERS} "
                                  "walkers per call")
    _soft_routes_grad_limits("soft_routes_backward", H, W, S, N, K)
    dev = _field_device(maps)
    for name, x in (("starts", idx), ("routes", routes), ("route_lengths", route_lengths), ("status", status), ("grad_log_probs", grad_log_probs)):
        if x.device != dev:
            raise ValueError(f"the maps live on {dev}, {name} on {x.device}: they must share a device")
    lib = _field_lib("nastar_soft_routes_backward", "nastar_soft_routes_grad.h")
    if not torch.is_tensor(tape) or tape.dtype != torch.uint8 or tape.device != dev or not tape.is_contiguous():
        raise ValueError(f"tape must be the contiguous uint8 tensor soft_fields_forward(..., tape=True) returned, on {dev}")
    with torch.no_grad():
        cost, goal, passable = (_maps3(m.detach()) for m in maps)
        idx, rows, lens, st = idx.contiguous(), routes.detach().contiguous(), route_lengths.detach().contiguous(), status.detach().contiguous()
        up = grad_log_probs.detach().contiguous()
        grad = torch.empty((B, H, W), dtype=torch.float32, device=dev)
        map_status = torch.empty((B,), dtype=torch.int32, device=dev)
        ws_bytes = int(lib.nastar_soft_routes_grad_workspace_bytes(B, H, W))
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            rc = lib.nastar_soft_routes_backward(cost.data_ptr(), goal.data_ptr(), passable.data_ptr(), tape.data_ptr(), tape.numel(),
                                                 idx.data_ptr(), rows.data_ptr(), cap, lens.data_ptr(), st.data_ptr(), up.data_ptr(), B, S, N, H, W,
                                                 mask, t, K, grad.data_ptr(), map_status.data_ptr(), ws.data_ptr(), ws_bytes, _stream_ptr(dev))
        _native.check(rc, "nastar_soft_routes_backward")
    return grad, map_status


class _SoftRoutesNode(torch.autograd.Function):
    """``soft_routes`` as an autograd node whose ONE differentiable output is ``log_probs``: the forward is the evaluation call (the
    field with its tape, then the walkers), the backward one call of ``nastar_soft_routes_backward`` with the upstream gradient of
    ``log_probs``; the gradient goes to ``cost_maps`` alone.  ``idx``: the checked [B,S] int32 start cells; ``call``: the checked
    ``(tau, horizon, num_samples, seed, neighbor_mask, max_route_len, visits)``.  What the backward reads is saved under autograd's version
    check: an in-place change of ``routes`` or ``cost_maps`` in between raises torch's own error."""

    @staticmethod
    def forward(ctx, cost_maps, goal_maps, obstacles_maps, idx, uniforms, call):
        tau, K, N, seed, mask, max_route_len, visits = call
        out, tape = _soft_routes_run(False, cost_maps, goal_maps, obstacles_maps, idx, tau, K, N, seed, mask, max_route_len, visits, uniforms)
        ctx.save_for_backward(cost_maps, goal_maps, obstacles_maps, tape, idx, out.routes, out.route_lengths, out.status)
        ctx.call = (tau, K, mask)
        ctx.mark_non_differentiable(*(x for x in out if x is not None and x is not out.log_probs))
        ctx.set_materialize_grads(False)
        return tuple(out)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        g_logp = grads[3]  # (SoftRoutes: routes, route_lengths, route_costs, log_probs, ...)
        if g_logp is None or not ctx.needs_input_grad[0]:
            return (None,) * 6
        cost_maps, goal_maps, obstacles_maps, tape, idx, routes, lengths, status = ctx.saved_tensors
        grad = soft_routes_backward(cost_maps, goal_maps, obstacles_maps, tape, idx, routes, lengths, status, g_logp, *ctx.call)[0]
        return (_widen_grad(grad, tuple(cost_maps.shape)), None, None, None, None, None)


def route_score_loss(log_probs: torch.Tensor, rewards: torch.Tensor, status: torch.Tensor, baseline="mean") -> torch.Tensor:
    """The surrogate whose gradient is the REINFORCE (score-function) estimate of the gradient of the expected reward -> a scalar: the mean,
    over the walkers of the queries with ``status == 0``, of ``(rewards - baseline).detach() * log_probs``.  ``log_probs`` [B,S,N] of
    ``soft_routes(..., differentiable=True)``; ``rewards`` [B,S,N]: any number per sampled route -- its length, its clearance, a
    simulator's verdict -- and no function of the costs; ``status`` [B,S] of the same call.  ``baseline``: "mean" (per query, over its N
    samples), None, or a tensor that broadcasts against ``rewards``.  A failed query has ``log_probs`` of -inf and whatever reward the
    caller computed from rows of -1: its entries are MASKED with ``torch.where`` -- a product with 0 would make NaN of them, in the value
    and in the gradient -- so they add nothing and receive a zero gradient; with no ok walker at all the loss is 0.  Plain torch: no
    kernel, no host read."""
    if not torch.is_tensor(log_probs) or log_probs.ndim != 3 or not log_probs.is_floating_point():
        raise ValueError(f"log_probs must be a float [B,S,N] tensor, got {tuple(log_probs.shape) if torch.is_tensor(log_probs) else type(log_probs).__name__}")
    if not torch.is_tensor(rewards) or tuple(rewards.shape) != tuple(log_probs.shape):
        raise ValueError(f"rewards must be a tensor of the shape of log_probs {tuple(log_probs.shape)}, got "
                         f"{tuple(rewards.shape) if torch.is_tensor(rewards) else type(rewards).__name__}")
    if not torch.is_tensor(status) or tuple(status.shape) != tuple(log_probs.shape[:2]) or status.is_floating_point():
        raise ValueError(f"status must be the integer [B,S] tensor of the call, {tuple(log_probs.shape[:2])}, got "
                         f"{tuple(status.shape) if torch.is_tensor(status) else type(status).__name__}")
    ok = (status == 0).unsqueeze(-1).expand_as(log_probs)
    r = torch.where(ok, rewards.detach().to(log_probs.dtype), torch.zeros_like(log_probs))
    if isinstance(baseline, str) and baseline == "mean":
        base = r.mean(-1, keepdim=True)
    elif baseline is None:
        base = torch.zeros_like(r)
    elif torch.is_tensor(baseline):
        base = baseline.detach().to(log_probs.dtype)
    else:
        raise ValueError(f'baseline must be "mean", None or a tensor, got {baseline!r}')
    zero = torch.zeros_like(log_probs)
    advantage = torch.where(ok, r - base, zero).detach()
    terms = advantage * torch.where(ok, log_probs, zero)
    return terms.sum() / ok.sum().clamp(min=1).to(log_probs.dtype)


# ---- include/nastar_soft_routes_tiled.h: the same samples from the tiled field's checkpointed tape
def soft_routes_tiled_from_tape(cost_maps: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor, tape: torch.Tensor,
                                starts: torch.Tensor, tau: float, horizon: Optional[int] = None, num_samples: int = 1, seed: int = 0,
                                neighbor_mask: Optional[int] = None, max_route_len: Optional[int] = None, visits: bool = False,
                                uniforms: Optional[torch.Tensor] = None, checkpoint_every: Optional[int] = None):
    """``nastar_soft_routes_tiled`` as it is (include/nastar_soft_routes_tiled.h) -> ``(routes, route_lengths, route_costs, log_probs,
    visits or None, status)``: the maps, ``tau``, ``horizon``, mask and ``checkpoint_every`` of the ``soft_fields_tiled_forward(...,
    tape=True)`` call that wrote ``tape``.  On the current stream: a prepare and a clear launch, then per segment of the tape the
    forward's sweeps that rebuild its planes and one launch of walkers; nothing is read back.  With ``max_route_len`` below
    ``horizon + 1`` the walk is replayed for the stores and every segment is rebuilt TWICE; None = rows of ``horizon + 1`` cells never
    pays that.  The other arguments are ``soft_routes_from_tape``'s.  What ``soft_routes_tiled`` runs behind its forward."""
    return _soft_routes_from_tape(True, cost_maps, goal_maps, obstacles_maps, tape, starts, tau, horizon, num_samples, seed, neighbor_mask,
                                  max_route_len, visits, uniforms, checkpoint_every=checkpoint_every)


def soft_routes_tiled(cost_maps: torch.Tensor, goal_maps: torch.Tensor, obstacles_maps: torch.Tensor, starts: torch.Tensor, tau: float,
                      horizon: Optional[int] = None, num_samples: int = 1, seed: Optional[int] = None, neighbor_mask: Optional[int] = None,
                      max_route_len: Optional[int] = None, visits: bool = False, uniforms: Optional[torch.Tensor] = None,
                      differentiable: bool = False, checkpoint_every: Optional[int] = None) -> SoftRoutes:
    """``soft_routes`` for maps of up to ``SOFT_FIELDS_TILED_MAX_CELLS`` cells (1024x1152: every map size the search takes), from the
    tiled field's checkpointed tape (include/nastar_soft_routes_tiled.h) -> ``SoftRoutes``.  The same definition, the same arguments and,
    on the maps both take, the same BITS in every output, whatever ``checkpoint_every`` is (None = ceil(sqrt(horizon)); 1 keeps every
    plane); NotImplementedError above the limit, before anything is launched.

    An EVALUATION call on the current stream: ``soft_cost_to_go_tiled``'s launches with the tape, then about one more forward -- the
    sweeps that rebuild each segment of the tape, top down -- with one launch of walkers per segment; a walker lives in a workspace
    between two launches.  With ``max_route_len`` below ``horizon + 1`` the walk is replayed, first for the lengths, then for the
    stores, and every segment is rebuilt TWICE; the default rows of ``horizon + 1`` cells never pay that.  Detached outputs, nothing is
    read back, nothing raises for a failed query or a bad map: read ``status`` and ``map_status``.  ``differentiable=True`` is not built
    for the tiled tape: NotImplementedError."""
    return _soft_routes(True, cost_maps, goal_maps, obstacles_maps, starts, tau, horizon, num_samples, seed, neighbor_mask, max_route_len, visits,
                        uniforms, checkpoint_every, differentiable)
