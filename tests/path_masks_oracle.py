"""The exact shortest path as a 0/1 mask and its blackbox gradient in numpy: the DEFINITION of include/nastar_path_masks.h (DESIGN.md
section 2, item 6j).

Forward: the field of ``fields_oracle.field``, the successor and the route of ``field_routes_oracle``, a scatter of the route's cells.
Backward: the perturbation in float32 exactly as the header writes it -- fl32(lambda * g), fl32(that + cost), the clamp at min_cost, a NaN
staying a NaN --, a second forward, and (y_lambda - y) * fl32(1 / lambda).
"""
import os
import sys
from typing import NamedTuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import field_routes_oracle as RO  # noqa: E402
import fields_oracle as FO  # noqa: E402
from heuristic_oracle import MOORE8  # noqa: E402

f32 = np.float32
STATUS_OK, STATUS_BAD_SHAPE, STATUS_UNSOLVABLE, STATUS_BAD_COST, STATUS_PLATEAU = 0, 1, 3, 9, 11


class Path(NamedTuple):
    mask: np.ndarray   # [H,W] f32 0/1; all-zero for a failed map
    cost: np.float32   # the field at the start; +inf for a failed map
    status: int
    cells: list        # the route in travel order; [] for a failed map


def start_index(start_map) -> int:
    """the highest-index non-zero cell of a start map, -1 for an all-zero one"""
    nz = np.flatnonzero(np.asarray(start_map).reshape(-1) != 0)
    return int(nz[-1]) if len(nz) else -1


def path(cost, goal, passable, n0, mask=MOORE8) -> Path:
    """[H,W] arrays and ONE flat start index -> Path; the status codes in the header's order"""
    cost = np.asarray(cost, f32)
    H, W = cost.shape
    failed = lambda st: Path(np.zeros((H, W), f32), f32(np.inf), st, [])  # noqa: E731
    if not 0 <= n0 < H * W:
        return failed(STATUS_BAD_SHAPE)
    dist, _, st = FO.field(cost, goal, passable, mask)
    if st != STATUS_OK:
        return failed(st)                                   # BAD_COST before a missing goal: the order of fields_oracle
    cells, st = RO.route(dist, goal, RO.successors(dist, goal, passable, mask), n0)
    if st != STATUS_OK:
        return failed(st)
    y = np.zeros(H * W, f32)
    y[cells] = 1
    return Path(y.reshape(H, W), dist.reshape(-1)[n0], STATUS_OK, cells)


def perturbed(cost, grad_path, lam, min_cost) -> np.ndarray:
    """w' = max(fl32(fl32(lambda * g) + w), min_cost) in float32, two separately rounded operations; a NaN stays a NaN"""
    with np.errstate(invalid="ignore", over="ignore"):
        s = ((f32(lam) * np.asarray(grad_path, f32)).astype(f32) + np.asarray(cost, f32)).astype(f32)
        return np.where(np.isnan(s), s, np.fmax(s, f32(min_cost))).astype(f32)


def backward(cost, goal, passable, n0, grad_path, lam, min_cost, mask=MOORE8):
    """-> (grad_cost [H,W] f32, status of the perturbed solve, the forward Path, the perturbed Path or None).  A map whose forward failed
    has an all-zero gradient (nothing is solved, status 0); a map whose perturbed solve failed an all-NaN one."""
    fwd = path(cost, goal, passable, n0, mask)
    if fwd.status != STATUS_OK:
        return np.zeros_like(fwd.mask), STATUS_OK, fwd, None
    lamf = path(perturbed(cost, grad_path, lam, min_cost), goal, passable, n0, mask)
    if lamf.status != STATUS_OK:
        return np.full_like(fwd.mask, np.nan), lamf.status, fwd, lamf
    return ((lamf.mask - fwd.mask) * (f32(1) / f32(lam))).astype(f32), STATUS_OK, fwd, lamf


def batch(cost, goal, passable, starts, mask=MOORE8):
    """[B,H,W] arrays and [B] start indices -> (masks [B,H,W], costs [B], status [B] int32)"""
    out = [path(cost[b], goal[b], passable[b], int(starts[b]), mask) for b in range(len(cost))]
    return np.stack([o.mask for o in out]), np.array([o.cost for o in out], f32), np.array([o.status for o in out], np.int32)


def batch_backward(cost, goal, passable, starts, grad_path, lam, min_cost, mask=MOORE8):
    """-> (grad_cost [B,H,W], status [B] int32, changed [B] bool: y_lambda differs from y, clamped [B] bool: the clamp bound on a passable cell)"""
    out = [backward(cost[b], goal[b], passable[b], int(starts[b]), grad_path[b], lam, min_cost, mask) for b in range(len(cost))]
    changed = np.array([o[3] is not None and o[3].status == 0 and not np.array_equal(o[3].mask, o[2].mask) for o in out])
    with np.errstate(invalid="ignore"):
        raw = ((f32(lam) * np.asarray(grad_path, f32)).astype(f32) + np.asarray(cost, f32)).astype(f32)
        clamped = ((raw < f32(min_cost)) & (np.asarray(passable) != 0)).reshape(len(out), -1).any(1)
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int32), changed, clamped
