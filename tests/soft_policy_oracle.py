"""The log-policy of the entropy-regularised cost-to-go field and the vector-Jacobian product through it, in numpy: the DEFINITION of
include/nastar_soft_policy.h, built on tests/soft_fields_oracle.py.

logpi_K(a|n) = -(V_{K-1}(m_a) - min) / tau - ln(S) on the cells live at K and the actions of Act(n), -inf elsewhere.  Its adjoint reaches
plane K-1 as Z(m) = -(1 / tau) * sum over the predecessors n of m, live at K, of (GL(a,n) - pi_K(a|n) gsum(n)); from there on it is the
field's own adjoint over the K-1 planes below, which ``soft_field_grad`` walks: the planes V_0 .. V_{K-1} of the horizon-K field ARE the
field of horizon K-1.  ``dtype=np.float64`` is the reference; ``dtype=np.float32`` runs the same statements in float32 (the sum over k
stays in float64) -- the scale a float32 kernel is measured against.
"""
import os
import sys
from typing import NamedTuple, Optional

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import soft_fields_oracle as SO  # noqa: E402
from fields_oracle import ACTION_MOVES  # noqa: E402
from heuristic_oracle import MOORE8, offsets  # noqa: E402

f32, f64 = np.float32, np.float64


class LogPolicy(NamedTuple):
    logp: np.ndarray             # [8,H,W]: logpi_K in ACTION_MOVES order, -inf outside (live at K, Act)
    act: np.ndarray              # [8,H,W] bool: n live at K and a in Act(n) -- where logp is finite and where GL is read
    field: SO.SoftField


def _row_major(mask):
    """the moves of the mask in the row-major order of their offsets: (-1,-1) (-1,0) (-1,1) (0,-1) ..."""
    return sorted(offsets(mask))


def log_policy(cost, goal, passable, tau, horizon, mask=MOORE8, dtype=f64) -> LogPolicy:
    """[H,W] arrays -> LogPolicy, every statement in ``dtype``"""
    dt = np.dtype(dtype).type
    fld = SO.soft_field(cost, goal, passable, tau, horizon, mask, dtype)
    H, W = fld.dist.shape
    logp = np.full((8, H, W), -np.inf, dtype)
    act = np.zeros((8, H, W), bool)
    if fld.planes is None:       # a BAD_COST map
        return LogPolicy(logp, act, fld)
    moves = _row_major(mask)
    live = (np.asarray(passable) != 0) & (np.asarray(goal) == 0) & np.isfinite(fld.planes[horizon])
    X, base, S, fin = SO._softmin(fld.planes[horizon - 1], moves, tau)
    for j, mv in enumerate(moves):
        a = ACTION_MOVES.index(mv)
        act[a] = live & fin & np.isfinite(X[j])
        with np.errstate(invalid="ignore"):
            logp[a] = np.where(act[a], -(X[j] - base) / dt(tau) - np.log(S), dt(-np.inf))
    return LogPolicy(logp, act, fld)


class PolicyGrad(NamedTuple):
    grad: np.ndarray             # [H,W] float64: the gradient with respect to the costs, from both seeds
    field_part: np.ndarray       # [H,W] float64: what the seed G of the field gives (``soft_field_grad``)
    policy_part: np.ndarray      # [H,W] float64: what the seed GL of the log-policy gives
    ever: np.ndarray             # [H,W] bool: live at some step 1..K
    act: np.ndarray              # [8,H,W] bool


def soft_policy_grad(cost, goal, passable, G: Optional[np.ndarray], GL: Optional[np.ndarray], tau, horizon, mask=MOORE8,
                     dtype=f64) -> PolicyGrad:
    """the vector-Jacobian product of (``soft_field(...).dist``, ``log_policy(...).logp``) with the upstream gradients G [H,W] and GL
    [8,H,W] (None = zeros); Z, pi and A in ``dtype``, the sums over k in float64"""
    dt = np.dtype(dtype).type
    lp = log_policy(cost, goal, passable, tau, horizon, mask, dtype)
    H, W = lp.field.dist.shape
    fg = SO.soft_field_grad(cost, goal, passable, np.zeros((H, W)) if G is None else G, tau, horizon, mask, dtype)
    part = np.zeros((H, W), f64)
    if GL is not None and lp.field.planes is not None and horizon >= 2:
        moves = _row_major(mask)
        X, base, S, fin = SO._softmin(lp.field.planes[horizon - 1], moves, tau)
        gl = [np.where(lp.act[ACTION_MOVES.index(mv)], np.asarray(GL, dtype)[ACTION_MOVES.index(mv)], dt(0)) for mv in moves]  # where: never a product
        gsum = np.zeros((H, W), dtype)
        for g in gl:
            gsum = (gsum + g).astype(dtype)
        Z = np.zeros((H, W), dtype)
        for j, (dy, dx) in sorted(enumerate(moves), key=lambda t: (-t[1][0], -t[1][1])):   # the predecessor's position, row-major
            with np.errstate(under="ignore"):
                pi = np.exp(-(X[j] - base) / dt(tau)) / S
            term = np.where(lp.act[ACTION_MOVES.index((dy, dx))], gl[j] - pi * gsum, dt(0)).astype(dtype)
            Z = (Z + SO._shift(term, -dy, -dx, dt(0))).astype(dtype)                      # held at n, moved to m = n + (dy, dx)
        Z = (-Z / dt(tau)).astype(dtype)
        # plane K-1 onwards: the field's own adjoint (it takes Z on the cells live at K-1 only: a goal absorbs it)
        part = SO.soft_field_grad(cost, goal, passable, Z, tau, horizon - 1, mask, dtype).grad
    return PolicyGrad(fg.grad + part, fg.grad, part, fg.ever, lp.act)


def log_policies(cost, goal, passable, tau, horizon, mask=MOORE8, dtype=f64):
    """[B,(1,)H,W] arrays -> (logp [B,8,H,W], act [B,8,H,W] bool)"""
    c, g, p = SO._b3(cost), SO._b3(goal), SO._b3(passable)
    out = [log_policy(c[b], g[b], p[b], tau, horizon, mask, dtype) for b in range(c.shape[0])]
    return np.stack([o.logp for o in out]), np.stack([o.act for o in out])


def soft_policy_grads(cost, goal, passable, G, GL, tau, horizon, mask=MOORE8, dtype=f64):
    """[B,(1,)H,W] arrays, G [B,H,W] or None, GL [B,8,H,W] or None -> (grad [B,H,W] float64, ever live [B,H,W] bool)"""
    c, g, p = SO._b3(cost), SO._b3(goal), SO._b3(passable)
    out = [soft_policy_grad(c[b], g[b], p[b], None if G is None else SO._b3(G)[b], None if GL is None else np.asarray(GL)[b], tau, horizon,
                            mask, dtype) for b in range(c.shape[0])]
    return np.stack([o.grad for o in out]), np.stack([o.ever for o in out])


def upstream(seed, act):
    """a random upstream gradient of the log-policy with a NaN on every entry outside (live at K, Act)"""
    GL = np.random.default_rng(seed).standard_normal(act.shape)
    return np.where(act, GL, np.nan)


def nll(logp, act, opt_policies):
    """the per-cell imitation loss of one batch in float64: logp, act, opt_policies [B,8,H,W] -> (loss [B], its gradient with respect
    to logp [B,8,H,W], 0 outside the picked entries)"""
    w = np.asarray(opt_policies, f64)
    counted = act.any(1) & (w != 0).any(1)
    pick = (w != 0) & counted[:, None]
    n = np.maximum(counted.sum((1, 2)), 1).astype(f64)
    loss = -(w * np.where(pick, logp, 0.0)).sum((1, 2, 3)) / n
    return loss, np.where(pick, -w, 0.0) / n[:, None, None, None]


# Relative to max |float64 gradient| of a case.  Measured on SO.SHAPE_CASES x SO.sweep_cases with the seed GL of ``upstream`` alone and
# together with a random G (printed by tests/test_soft_policy.py::test_float32_restatement_of_the_policy_gradient and, per case, by the
# GPU tests):
#   float32 restatement (this numpy) 1.693e-05, kernels 3.717e-05 (MI355X, the worst case of tests/test_soft_policy_gpu.py)
# The bound is 4 x the restatement's figure: headroom for the device's exp2 / log2 and the order of its sums (the margin
# soft_fields_oracle.py argues for), not for a wrong kernel.  As there, the figure is the float32 PLANES': GL - pi gsum cancels to the
# rounding of pi, an error of 4e-7 |V| / tau in a log-probability, and Z carries one more factor 1 / tau than the field's adjoint.
PGRAD_RTOL = 4 * 1.693e-05
