"""CPU: the numpy restatement of the search with the heuristic as an input (tests/heuristic_oracle.py) pinned by the reference's vectors with
a replaced get_heuristic (tests/golden/heuristics/) and, fed the built-in heuristic, by oracle.forward() on Moore-8 vectors.  The GPU tests of
``forward(..., heuristic_maps=)`` (tests/test_heuristic_maps_gpu.py) rest on it."""
import numpy as np
import pytest

import golden_util as G
import heuristic_oracle as HO
from oracle import oracle as O


def test_the_vectors_cover_the_issue_table():
    names = set(HO.names())
    assert {"zero32_binary_g050", "zero32_ucost_g050", "w2_64_ucost_g050", "field20x45_ucost_g050", "field20x45_ucost_g020",
            "coupled_field24_ucost_g050", "zero32_vn_ucost_g050", "noisy96_ucost_g050", "w2_140x150_ucost_g050", "grad_field32_train_T025",
            "grad_noisy80_eval_g050", "grad_coupled_field24_g050", "grad_h0only_field32_binary_g050", "grad_w2_140x150_eval_g050"} <= names
    assert (HO.load("zero32_ucost_g050").h0 == 0).all()
    assert HO.load("zero32_vn_ucost_g050").mask == HO.VON_NEUMANN
    assert HO.load("field20x45_ucost_g020").h0.min() < 0 and HO.load("field20x45_ucost_g020").g_ratio == 0.2
    g = HO.load("grad_h0only_field32_binary_g050")
    assert g.h0_only and g.grad_cost is None and g.grad_h0 is not None and np.array_equal(g.cost_maps, g.map_designs)
    for n in names:
        g = HO.load(n)
        assert g.sel_log.shape == (g.histories.shape[0], g.t_batch + 1) and np.isfinite(g.h0).all()
        if g.grad_cost is not None:  # the gradient identity the kernels rely on: dL/dh0 == dL/dcost, bit for bit, in the reference's autograd
            assert np.array_equal(g.grad_cost, g.grad_h0), n


@pytest.mark.parametrize("name", HO.names())
def test_restatement_reproduces_the_reference(name):
    g = HO.load(name)
    B = g.histories.shape[0]
    o = HO.search(g.cost_maps, g.start_maps, g.goal_maps, g.map_designs, g.h0, g.g_ratio, g.max_iters, g.mask, lockstep=B > 1)
    assert (o.status == 0).all()
    assert np.array_equal(o.histories, g.histories[:, 0]), "histories"
    assert np.array_equal(o.paths, g.paths[:, 0]), "paths"
    assert o.t_batch == g.t_batch
    for b in range(B):
        assert o.sel[b] == g.sel_log[b].tolist(), f"map {b}: selections"


@pytest.mark.parametrize("name", ["coupled_field24_ucost_g050", "grad_coupled_field24_g050"])
def test_the_coupled_vectors_leave_their_fixed_point(name):
    """the class the exact pipeline exists for: a map searched alone differs from its row in the batch"""
    g = HO.load(name)
    alone = HO.search(g.cost_maps, g.start_maps, g.goal_maps, g.map_designs, g.h0, g.g_ratio, g.max_iters, g.mask, lockstep=False)
    differs = [b for b in range(g.histories.shape[0]) if not np.array_equal(alone.histories[b], g.histories[b, 0])]
    assert differs and g.g_ratio == 0.5


@pytest.mark.parametrize("name", ["rand32_ucost_g050", "rand32_ucost_g080", "rand20x45_ucost_g050", "rand32_vanilla_g050", "fixture64_g020",
                                  "coupled_forward_g020", "coupled_signed_g050"])
def test_with_the_builtin_heuristic_it_is_the_oracle(name):
    g = G.load(name)
    B, _, H, W = g.map_designs.shape
    h0 = np.stack([O.heuristic(H, W, *divmod(int(g.goal_maps[b].reshape(-1).argmax()), W)) for b in range(B)])
    max_iters = O.max_iters_for(W, g.Tmax, g.training)
    ref = O.forward(g.cost_maps, g.start_maps, g.goal_maps, g.map_designs, g.g_ratio, max_iters, mode="dense", want_log=True)
    o = HO.search(g.cost_maps, g.start_maps, g.goal_maps, g.map_designs, h0, g.g_ratio, max_iters, HO.MOORE8, lockstep=B > 1)
    assert np.array_equal(o.histories, ref.histories) and np.array_equal(o.paths, ref.paths)
    assert o.t_batch == ref.t_batch
    for b in range(B):
        assert o.sel[b] == ref.sel_log[b, :len(o.sel[b])].tolist()
        assert len(o.sel[b]) == ref.t_batch + 1


@pytest.mark.parametrize("mask", [HO.MOORE8, HO.VON_NEUMANN, 0b000001011])
def test_with_the_builtin_heuristic_and_a_mask_it_is_the_masked_oracle(mask):
    g = G.load("rand32_ucost_g050")
    B, _, H, W = g.map_designs.shape
    h0 = np.stack([O.heuristic(H, W, *divmod(int(g.goal_maps[b].reshape(-1).argmax()), W)) for b in range(B)])
    ref = O.forward(g.cost_maps, g.start_maps, g.goal_maps, g.map_designs, g.g_ratio, W * W, mode="sm", want_log=True, neighbor_mask=mask)
    o = HO.search(g.cost_maps, g.start_maps, g.goal_maps, g.map_designs, h0, g.g_ratio, W * W, mask, lockstep=False)
    solved = o.status == 0
    assert np.array_equal(solved, np.asarray(ref.map_status) == 0)
    assert np.array_equal(o.histories[solved], ref.histories[solved]) and np.array_equal(o.paths[solved], ref.paths[solved])
    assert np.array_equal(o.iters[solved], ref.iters[solved])
