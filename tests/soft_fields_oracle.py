"""The entropy-regularised (soft-min) cost-to-go field over a finite horizon, its soft policy and its adjoint in numpy: the DEFINITION of
include/nastar_soft_fields.h.

A move n -> m = n + off, off in ``heuristic_oracle.offsets(mask)``, m inside the map and passable, costs cost[n] (the cell being left).
V_0 = 0 on passable goals, +inf elsewhere; V_k(n) = cost[n] + softmin_tau over the moves of V_{k-1}(m), from plane k-1 only; the output is
V_K with 0 on every goal (a goal on an obstacle too).  The adjoint walks the planes back: grad += A_k, A_{k-1}(m) = sum over n of
pi_k(m|n) A_k(n) on the cells live at k-1, with pi normalised directly.  ``dtype=np.float64`` is the reference; ``dtype=np.float32`` runs
the same statements in float32 (the sum over k stays in float64, as the header says) -- the scale a float32 kernel is measured against.
"""
import os
import sys
from typing import NamedTuple, Optional

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fields_oracle import ACTION_MOVES  # noqa: E402
from heuristic_oracle import MOORE8, offsets  # noqa: E402

f32, f64 = np.float32, np.float64
STATUS_OK, STATUS_NO_GOAL, STATUS_BAD_COST = 0, 3, 9
DIRECTED = 0x00A  # right (0,1) and down (1,0) only: bit a*3+b <=> offset (1-a, 1-b)


def default_horizon(H: int, W: int) -> int:
    return 2 * (H + W)


def _shift(x, dy, dx, fill):
    """y[r, c] = x[r + dy, c + dx], ``fill`` outside the map"""
    H, W = x.shape
    pad = np.full((H + 2, W + 2), fill, x.dtype)
    pad[1:-1, 1:-1] = x
    return pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]


class SoftField(NamedTuple):
    dist: np.ndarray             # [H,W]: V_K, 0 on every goal, +inf on obstacles and where no goal lies within K moves
    policy: np.ndarray           # [8,H,W]: pi_K in ACTION_MOVES order
    status: int
    planes: Optional[list]       # [V_0 .. V_K] as the recursion reads them (a goal on an obstacle is +inf there); None for a BAD_COST map


def _softmin(V, moves, tau):
    """-> (X [n,H,W] the targets' values, m [H,W] their minimum, S [H,W] the sum of exp(-(x - m) / tau), fin [H,W] bool)"""
    dt = V.dtype.type
    X = np.stack([_shift(V, dy, dx, dt(np.inf)) for dy, dx in moves]) if moves else np.full((1,) + V.shape, np.inf, V.dtype)
    m = X.min(0)
    fin = np.isfinite(m)
    base = np.where(fin, m, dt(0))
    with np.errstate(under="ignore"):
        S = np.exp(-(X - base) / dt(tau)).sum(0, dtype=V.dtype)
    return X, base, np.where(fin, S, dt(1)), fin


def soft_field(cost, goal, passable, tau, horizon, mask=MOORE8, dtype=f64) -> SoftField:
    """[H,W] arrays -> SoftField, every statement in ``dtype``"""
    dt = np.dtype(dtype).type
    cost, ok, gl = np.asarray(cost, f32).astype(dtype), np.asarray(passable) != 0, np.asarray(goal) != 0
    H, W = cost.shape
    inf = np.full((H, W), np.inf, dtype)
    if (ok & ~(cost >= 0)).any():
        return SoftField(inf, np.zeros((8, H, W), dtype), STATUS_BAD_COST, None)
    moves = offsets(mask)
    V = np.where(gl & ok, dt(0), inf)
    planes = [V]
    for _ in range(horizon):
        _, base, S, fin = _softmin(V, moves, tau)
        with np.errstate(invalid="ignore"):
            soft = np.where(fin, base - dt(tau) * np.log(S), inf)
            V = np.where(gl & ok, dt(0), np.where(ok, cost + soft, inf)).astype(dtype)
        planes.append(V)
    pol = np.zeros((8, H, W), dtype)
    X, base, S, fin = _softmin(planes[-2], moves, tau)
    live = ok & ~gl & np.isfinite(V)
    for j, mv in enumerate(moves):
        with np.errstate(under="ignore"):
            pol[ACTION_MOVES.index(mv)] = np.where(live & fin, np.exp(-(X[j] - base) / dt(tau)) / S, dt(0))
    return SoftField(np.where(gl, dt(0), V), pol, STATUS_OK if gl.any() else STATUS_NO_GOAL, planes)


class SoftGrad(NamedTuple):
    grad: np.ndarray    # [H,W] float64: the sum over k of A_k (0 on a cell that was never live)
    ever: np.ndarray    # [H,W] bool: live at some step 1..K
    live: np.ndarray    # [H,W] bool: live at K -- where the upstream gradient is read


def soft_field_grad(cost, goal, passable, G, tau, horizon, mask=MOORE8, dtype=f64) -> SoftGrad:
    """the vector-Jacobian product of ``soft_field(...).dist`` with the upstream gradient G [H,W]; A and pi in ``dtype``, the sum in float64"""
    dt = np.dtype(dtype).type
    fld = soft_field(cost, goal, passable, tau, horizon, mask, dtype)
    H, W = fld.dist.shape
    if fld.planes is None:
        return SoftGrad(np.zeros((H, W)), np.zeros((H, W), bool), np.zeros((H, W), bool))
    elig = (np.asarray(passable) != 0) & (np.asarray(goal) == 0)
    moves = offsets(mask)
    live = [elig & np.isfinite(V) for V in fld.planes]
    A = np.where(live[horizon], np.asarray(G, dtype), dt(0))  # (where, not a product: what is not live is never read)
    grad = np.zeros((H, W), f64)
    ever = np.zeros((H, W), bool)
    for k in range(horizon, 0, -1):
        grad += A
        ever |= live[k]
        X, base, S, fin = _softmin(fld.planes[k - 1], moves, tau)
        below = np.zeros((H, W), dtype)
        for j, (dy, dx) in enumerate(moves):
            with np.errstate(under="ignore"):
                flow = np.where(fin, np.exp(-(X[j] - base) / dt(tau)) / S * A, dt(0)).astype(dtype)  # pi_k(m|n) A_k(n), held at n
            below += _shift(flow, -dy, -dx, dt(0))                                                    # ... moved to m = n + (dy, dx)
        A = np.where(live[k - 1], below, dt(0))
    return SoftGrad(grad, ever, live[horizon])


def hops(goal, passable, mask=MOORE8) -> np.ndarray:
    """[H,W] int64: the fewest moves from a cell to a passable goal (0 there), -1 where there is no route"""
    ok, gl = np.asarray(passable) != 0, np.asarray(goal) != 0
    moves = offsets(mask)
    d = np.where(gl & ok, 0, -1).astype(np.int64)
    k = 0
    while True:
        k += 1
        near = np.zeros(d.shape, bool)
        for dy, dx in moves:
            near |= _shift(d, dy, dx, -1) >= 0
        new = ok & (d < 0) & near
        if not new.any():
            return d
        d[new] = k


def _b3(a):
    a = np.asarray(a)
    return a.reshape((a.shape[0],) + a.shape[-2:])


def soft_fields(cost, goal, passable, tau, horizon, mask=MOORE8, dtype=f64):
    """[B,(1,)H,W] arrays -> (dist [B,H,W], policies [B,8,H,W], status [B] int32)"""
    c, g, p = _b3(cost), _b3(goal), _b3(passable)
    out = [soft_field(c[b], g[b], p[b], tau, horizon, mask, dtype) for b in range(c.shape[0])]
    return np.stack([o.dist for o in out]), np.stack([o.policy for o in out]), np.array([o.status for o in out], np.int32)


def soft_field_grads(cost, goal, passable, G, tau, horizon, mask=MOORE8, dtype=f64):
    """[B,(1,)H,W] arrays -> (grad [B,H,W] float64, ever live [B,H,W] bool, live at K [B,H,W] bool)"""
    c, g, p, u = _b3(cost), _b3(goal), _b3(passable), _b3(G)
    out = [soft_field_grad(c[b], g[b], p[b], u[b], tau, horizon, mask, dtype) for b in range(c.shape[0])]
    return np.stack([o.grad for o in out]), np.stack([o.ever for o in out]), np.stack([o.live for o in out])


# ---- the cases the CPU and the GPU tests share, and the bounds they hold the float32 results to ---------------------------------------------
# (H, W, B, seed): a goal alone; one row, one column; fewer cells than a wavefront, B = 3 with an odd H*W (unaligned map bases); 256 cells,
# the most one wavefront takes, and 257, the first map of the 256-lane workgroup; 1023 cells, one short of the 1024 that workgroup takes;
# 1056 cells, the 1024-lane workgroup with a ragged second round
SHAPE_CASES = ((1, 1, 1, 1), (1, 9, 1, 2), (9, 1, 1, 3), (5, 7, 3, 4), (16, 16, 2, 7), (1, 257, 1, 8), (31, 33, 3, 5), (32, 33, 2, 6))
TAUS = (1.0, 0.02)  # V goes far below 0; cost / tau up to 50 per step: exp underflows, soft is nearly hard
MASKS = (MOORE8, 0x0AA, DIRECTED)

# Relative to max |float64 value| of a case (max |V| over the finite cells; max |grad|).  Measured on the cases above (printed by
# test_float32_restatement_stays_inside_the_committed_bounds and, per case, by the GPU tests):
#   forward   float32 restatement 4.20e-07 (this numpy), kernels 5.33e-07 (MI355X, the worst case of tests/test_soft_fields_gpu.py)
#   backward  float32 restatement 1.70e-05,              kernels 7.69e-06
# The bound is 4 x the larger of the two: the device's exp2 / log2 and the order of its sums differ from numpy's by a few ulp per sweep,
# and 4 x is headroom for another machine's libm, not for a wrong kernel.  The backward's figure is the float32 TAPE's, not the adjoint's:
# pi is exp(-(V_{k-1}(m) - min) / tau), so an error of 4e-7 * |V| in a plane is an error of 4e-7 * |V| / tau in a log-probability, and the
# adjoint passes through K of them -- the restatement shows it without any kernel (and more of it than the kernels, which take the
# difference of two planes' values in units of tau ln 2 before anything is scaled).
FWD_RTOL = 4 * 5.33e-07
BWD_RTOL = 4 * 1.70e-05


def sweep_cases(goal, passable):
    """the (horizon, tau, mask) of one shape: horizons 1, one short of the farthest cell's hop distance, and 2 * (H + W)"""
    H, W = np.asarray(goal).shape
    for mask in MASKS:
        far = int(hops(goal, passable, mask).max())
        for K in sorted({1, max(1, far - 1), default_horizon(H, W)}):
            for tau in TAUS:
                yield K, tau, mask


def rel_err(got, ref) -> float:
    """max |got - ref| over the cells where ref is finite, relative to max |ref| there; 0 for a case of zeros"""
    ref = np.asarray(ref, f64)
    fin = np.isfinite(ref)
    scale = np.abs(ref[fin]).max() if fin.any() else 0.0
    return float(np.abs(np.asarray(got, f64)[fin] - ref[fin]).max() / scale) if scale > 0 else 0.0


def random_maps(seed, B, H, W, p_obstacle=0.25, lo=0.1, hi=1.0):
    """cost U(lo, hi), passable (f32 0/1), goal (one-hot f32 on a passable cell): [B,H,W] each"""
    rng = np.random.default_rng(seed)
    cost = (lo + (hi - lo) * rng.random((B, H, W))).astype(f32)
    passable = (rng.random((B, H, W)) >= p_obstacle).astype(f32)
    goal = np.zeros((B, H, W), f32)
    for b in range(B):
        y, x = rng.integers(0, H), rng.integers(0, W)
        passable[b, y, x] = 1
        goal[b, y, x] = 1
    return cost, passable, goal
