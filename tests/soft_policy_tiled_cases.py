"""The cases tests/test_soft_policy_tiled.py (CPU) and tests/test_soft_policy_tiled_gpu.py share: the maps above the one-workgroup limits
(those of tests/soft_fields_tiled_cases.py) with the upstream gradients of the log-policy, the imitation-loss case, and the bound of the
gradient there.  The definitions are tests/soft_policy_oracle.py (``PO``) and tests/soft_fields_oracle.py (``SO``)."""
import functools

import numpy as np

import fields_oracle as FO
import soft_fields_oracle as SO
import soft_fields_tiled_cases as TC
import soft_policy_oracle as PO

f32, f64 = np.float32, np.float64

# Relative to max |float64 gradient| of a case.  ``PO.PGRAD_RTOL`` was measured on SO.SHAPE_CASES only (restatement 1.693e-05, kernels
# 3.717e-05 against 6.772e-05): too close for the larger maps and longer horizons here.  The float32 restatement of the policy gradient
# against float64 (tests/test_soft_policy_tiled.py::test_float32_restatement_of_the_tiled_policy_cases recomputes and prints it):
#   TC.ABOVE x TC.ABOVE_MASKS x SO.TAUS, GL of ``upstreams`` alone and with G    2.681e-05 (130x140, Moore-8, tau 0.02); kernels 2.111e-05
#   the loss case below, GL = the gradient of the loss                            3.793e-05 (tau 0.05);                  kernels 6.032e-05
# (kernels: MI355X, the worst case of tests/test_soft_policy_tiled_gpu.py, which prints every figure).  The bound is 4 x the larger figure, the rule of soft_policy_oracle.py: headroom for the device's exp2 / log2 and the order of its sums,
# not for a wrong kernel.
PTILED_RTOL = 4 * 3.793e-05


def upstreams(seed, act):
    """(G [B,H,W], GL [B,8,H,W]) for act [B,8,H,W]: random, with a NaN on every cell of G that is not live at K and on every entry of GL
    outside (live at K, Act)"""
    G = np.where(act.any(1), np.random.default_rng(seed + 100).standard_normal(act.any(1).shape), np.nan)
    return G, PO.upstream(seed, act)


# ---- the imitation loss: two 130x140 maps, K = 97, the optimal action of every cell as the demonstration --------------------------------------
LOSS_H, LOSS_W, LOSS_B, LOSS_SEED, LOSS_K = 130, 140, 2, 114, 97


def loss_maps():
    return TC.maps(LOSS_H, LOSS_W, LOSS_B, LOSS_SEED)


@functools.lru_cache(maxsize=None)
def loss_opt_policies():
    """the optimal policy of every cell [B,8,H,W] by the numpy definition of the exact field (what ``ops.cost_to_go_tiled`` returns)"""
    cost, passable, goal = loss_maps()
    return FO.fields(cost, goal, passable)[1]


def shown_outside_act(opt, act):
    """[B,H,W] bool: the cells live at K whose demonstrated action is not in Act -- its target has no goal within K - 1 moves"""
    return act.any(1) & ((np.asarray(opt) != 0) & ~act).any(1)


def restatement(cost, goal, passable, G, GL, tau, K, mask=SO.MOORE8):
    """the float32 restatement of the VJP against float64, GL alone and (with a G) both seeds: relative to the batch's max |gradient|, as the
    GPU tests measure the kernels (SO.rel_err)"""
    worst = 0.0
    for g in ([None] if G is None else [None, G]):
        a =PO.soft_policy_grads(cost, goal, passable, g, GL, tau, K, mask)[0]
        r = PO.soft_policy_grads(cost, goal, passable, g, GL, tau, K, mask, f32)[0]
        worst = max(worst, SO.rel_err(r, a))
    return worst
