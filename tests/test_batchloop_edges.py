"""CPU: the table of tests/batchloop_edges.py, held to what its class names say by the oracle alone -- every case reaches the branch of the exact
batch loop (nastar_forward_batchloop_finish, nastar_batchloop_tend_kernel) that tests/test_batchloop_edges_gpu.py runs it for.  No case is
skipped or filtered: a case that stops meeting its predicate fails here."""
import numpy as np
import pytest

import batchloop_edges as E


def _words(max_iters):
    return (max_iters + 31) // 32  # csrc/nastar_capi.hip bitmap_words_for


def test_the_names_known_at_collection_time_are_the_table():
    assert {k: [c.name for c in E.cases(k)] for k in "ABCDEF"} == E._NAMES
    assert all(E.cases(k) for k in "ABCDEF")  # every class is populated


def test_pools_hold_maps_whose_batch_run_is_not_the_map_alone():
    """the four configurations that reach the class and the signed one: each pool has maps that wander, and -- run as one batch --
    maps whose histories differ from the map alone"""
    for name in ("p8", "p16", "p12", "z16", "s16", "p32", "v12"):
        iters, wanders, differs = E.pool_runs(name) if name != "v12" else (None, None, E.expected(E.table()["F_masked_12x12_1100"]).differs)
        assert differs.sum() >= 50, (name, int(differs.sum()))
        if wanders is not None:
            assert (wanders[differs]).all() or name == "s16"  # (negative costs: a map may also leave its goal later than right after it)


@pytest.mark.parametrize("name", E.names("A"))
def test_large_batches_stride_over_maps_that_differ(name):
    c = E.table()[name]
    e = E.expected(c)
    B = len(c.maps)
    assert B > E.TEND_THREADS and c.max_iters is None and e.ok.all()
    if name == "A_16x16_marked_behind_1024":
        return  # (the test below)
    d = e.differs
    assert d[:E.TEND_THREADS].any() and d[E.TEND_THREADS:].any()  # on both sides of the tend kernel's stride


def test_the_maps_behind_the_stride_alone_decide_the_end_of_the_loop():
    """no map of the first 1024 wanders, and they finish by tmax: a tend kernel that counts or ANDs the first 1024 maps only finds no marked map, or
    ends the loop at tmax -- the batch loop ends later, in the next bitmap word"""
    c = E.table()["A_16x16_marked_behind_1024"]
    e = E.expected(c)
    wanders = E.pool_runs(c.pool)[1][list(c.maps)]
    assert len(c.maps) > E.TEND_THREADS and not wanders[:E.TEND_THREADS].any() and wanders[E.TEND_THREADS:].all()
    front = E.expected(c._replace(maps=c.maps[:E.TEND_THREADS]))
    assert front.tmax <= e.tmax and front.t_end == front.tmax and not front.differs.any()
    assert e.t_end > e.tmax and e.t_end >> 5 > e.tmax >> 5
    assert not e.differs[:E.TEND_THREADS].any() and e.differs[E.TEND_THREADS:].all()


def test_large_batches_cover_the_shapes_the_sizes_and_more_than_1024_marked_maps():
    A = E.cases("A")
    assert {len(c.maps) for c in A} >= {1025, 2100, 4096}
    assert {c.shape for c in A} == {(8, 8), (12, 12), (16, 16), (32, 32)}
    assert {c.g_ratio for c in A} == {0.0, 0.2, 0.5, 1.0}
    assert any(E.expected(c).differs[E.TEND_THREADS:].any() for c in A if len(c.maps) > 1025)
    c = E.table()["A_8x8_marked_1100"]
    wanders = E.pool_runs(c.pool)[1][list(c.maps)]
    assert wanders.sum() > E.TEND_THREADS and wanders[:E.TEND_THREADS].any() and wanders[E.TEND_THREADS:].any() and not wanders.all()
    assert E.expected(c).differs.sum() > E.TEND_THREADS


@pytest.mark.parametrize("name", E.names("B"))
def test_seam_cases_meet_their_predicates(name):
    c = E.table()[name]
    e = E.expected(c)
    assert 2 <= len(c.maps) <= 5 and E.pool_runs(c.pool)[1][list(c.maps)].all()  # every map of the sub-batch is a marked one
    assert E.SEAM_PREDICATES[c.seam](e.tmax, e.t_end, bool(e.differs.any())), (e.tmax, e.t_end)
    assert e.t_end < c.budget - 1  # (the loop ends by itself, not by the budget)


def test_seam_cases_name_every_seam():
    got = {c.seam: E.expected(c) for c in E.cases("B")}
    assert set(got) == set(E.SEAM_PREDICATES)
    assert got["tmax_bit0"].tmax & 31 == 0 and got["tmax_bit31"].tmax & 31 == 31 and got["w0_zero"].tmax < 32
    e = got["tend_same_word"]
    assert e.t_end > e.tmax and e.t_end >> 5 == e.tmax >> 5
    e = got["tend_later_word"]
    assert e.t_end >> 5 > e.tmax >> 5
    e = got["tend_is_tmax"]
    assert e.t_end == e.tmax and e.differs.any()


@pytest.mark.parametrize("name", E.names("C"))
def test_budget_cases_end_by_the_budget(name):
    c = E.table()[name]
    e = E.expected(c)
    natural = E._sub_batch(c.pool, c.maps)[1]
    assert natural > c.max_iters - 1 and e.t_end == c.max_iters - 1 == e.tmax  # the clamp; a budget-ended map is an ok map
    assert e.ok.all() and (e.sm_iters == c.max_iters).any() and e.differs.any()


def test_budget_cases_cover_the_word_edges_and_the_training_budget():
    assert sorted(c.max_iters for c in E.cases("C")) == [20, 31, 32, 33, 64, 65]
    assert int(0.25 * 16 * 16) == 64 and E.table()["C_budget_64"].shape == (16, 16)  # Tmax 0.25 in train mode is this case's budget


@pytest.mark.parametrize("name", E.names("D"))
def test_long_budget_cases_have_the_words_they_claim(name):
    c = E.table()[name]
    e = E.expected(c)
    nw = _words(c.max_iters) - (e.tmax >> 5)
    assert not c.want_log and e.differs.any() and e.ok.all()
    if c.nw:
        assert nw == c.nw and c.max_iters & 31  # (with a partial last word; 600000 steps fill theirs)
    assert c.seam == ("lds" if nw <= E.TEND_LDS_WORDS else "global")


def test_long_budget_cases_sit_on_both_sides_of_both_limits():
    nws = [c.nw for c in E.cases("D") if c.nw]
    assert nws == [E.TEND_LDS_WORDS, E.TEND_LDS_WORDS + 1, E.OLD_LDS_WORDS, E.OLD_LDS_WORDS + 1]
    assert E.TEND_LDS_WORDS * 4 + 16 == 64 * 1024 and E.OLD_LDS_WORDS * 4 == 64 * 1024
    assert {c.shape for c in E.cases("D") if c.max_iters == 600000} == {(12, 12), (80, 80)}
    e = E.expected(E.table()["D_12x12_600000"])
    assert e.t_end > e.tmax  # (the first goal-selection bit all maps share lies behind tmax: the mask of word 0 and ctz both count)


@pytest.mark.parametrize("name", E.names("E"))
def test_failed_maps_straddle_the_stride_and_hold_the_slowest_map(name):
    c = E.table()[name]
    e = E.expected(c)
    failed = np.flatnonzero(~e.ok)
    assert sorted(failed.tolist()) == sorted(c.walled + c.no_start) and len(c.no_start) >= 3
    assert 0.015 * len(c.maps) <= len(c.walled) <= 0.03 * len(c.maps)
    assert (e.sm_status[list(c.walled)] == E.STATUS_UNSOLVABLE).all()
    for group in (c.walled, c.no_start):
        assert min(group) < E.TEND_THREADS <= max(group)
    whole = E.expected(c._replace(walled=(), no_start=()))  # the same batch with every map taking part
    slowest = int(np.argmax(whole.sm_iters))
    assert slowest in c.walled and whole.sm_iters[slowest] - 1 == whole.tmax
    d = e.differs
    assert d[:E.TEND_THREADS].any() and d[E.TEND_THREADS:].any()
    if name == "E_16x16_2100":
        assert e.tmax < whole.tmax and e.t_end < whole.t_end  # without its slowest map the batch ends earlier


@pytest.mark.parametrize("name", E.names("F"))
def test_the_other_entry_points_have_work_to_do(name):
    c = E.table()[name]
    e = E.expected(c)
    assert len(c.maps) > E.TEND_THREADS and e.ok.all() and e.differs.sum() >= 50
    assert (c.mask == E.VON_NEUMANN) != c.zero_h and (not c.zero_h or c.g_ratio == 0.5)
