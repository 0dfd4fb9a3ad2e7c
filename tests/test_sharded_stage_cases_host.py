"""The cases of tests/test_gpu_sharded_stages.py hold what they were made for, and its references catch the mistakes they are there
for -- on the CPU, with the oracle's keys and the oracle's sums in the place of a rank (tests/sharded_stage_cases.py,
tests/select_reference.py).  No GPU needed.

Planted faults: the select's rank taken from the gathered buffer's length (``rank_from_count_all``), a list truncated at its capacity
and ranked by counting anyway (``truncated_list_ranked``: what ``select_finish_list`` did before the overflow was tested first), the
reduction in reverse rank order (``reverse_rank_order``), a partial whose second grid-stride trip is missing (``second_trip_missing``)."""
import numpy as np
import pytest

import select_cases as SC
import select_reference as S
import sharded_stage_cases as C
from oracle import ba_oracle as O

SELECT_NAMES = list(C.SELECT) + ["all-tied"]


def oracle_call(c, call):
    it, init, lam = C.CALLS[call]
    dbg = {}
    out, lam_out, _h, ntr = O.ba_iteration(it, c.states, c.cumrot, c.uv, c.xyz, c.ii, c.t, c.K, c.conf, lam, initialize=init, debug=dbg)
    return dbg, ntr


# ------------------------------------------------------------------------------------------------ slices
def test_slices_have_the_edges_they_were_cut_for():
    c = C.slices()
    assert (c.n, c.m) == (17, 91) and not np.array_equal(c.ii, np.sort(c.ii)), "rows in shuffled order"
    counts = np.bincount(c.ii, minlength=17)
    assert counts[:4].tolist() == [1, 16, 17, 33] and counts[9] == 0
    for ranks in C.SLICE_RANKS:
        p = C.slice_properties(c, ranks)
        assert sum(p["sizes"]) == c.m and max(p["sizes"]) - min(p["sizes"]) <= 1
        if ranks > 1:
            assert c.m % ranks != 0 and p["padded"], "m is no multiple of R: some slot ends in padding"
            assert p["split_poses"] and p["boundaries_inside_a_pose"], (ranks, p)
    p8 = C.slice_properties(c, 8)
    assert {1, 2} <= set(p8["inside_one_pose"]), p8
    for ranks in C.SLICE_RANKS[1:]:
        h = C.head(ranks + 1)
        p = C.slice_properties(h, ranks)
        assert p["sizes"] == [2] + [1] * (ranks - 1) and p["single_row"] == list(range(1, ranks)), p


def test_chain_needs_a_second_trip():
    c = C.chain()
    assert c.n == C.CHAIN_N and 27 * c.n > C.PACK_TRIP, "a chain that needs a second trip"
    counts = np.bincount(c.ii, minlength=c.n)
    assert (counts == 0).sum() >= 10 and counts.max() == 2 and c.m % C.CHAIN_RANKS != 0
    assert int(np.diff(c.t).max()) <= 64, "no long edge: the pose-chain sums have no slots of their own"
    # the entries behind the first trip are b of the last poses: they have rows
    first = (C.PACK_TRIP - 21 * c.n) // 6 + 1
    assert first < c.n - 1 and counts[first:].sum() >= 4


# ------------------------------------------------------------------------------------------------ select
@pytest.mark.parametrize("name", SELECT_NAMES)
def test_select_case_takes_its_branch_under_both_readings(name):
    c = C.select_case(name)
    keys = SC.oracle_keys(c)
    R = C.SELECT_RANKS
    sizes = np.diff(C.bounds(c.m, R))
    want = C.SELECT_BRANCH[name]
    flat = keys.reshape(-1)
    for m_local in sorted(set(int(s) for s in sizes)):
        p42, p31 = S.predict_gathered(flat, m_local), S.predict_gathered(flat, m_local, shift=31)
        assert p42["branch"] == want and p31["branch"] == want, (name, m_local, p42, p31)
        assert (p42["cnt"], p42["rank"]) == (p31["cnt"], p31["rank"]), "the list is the same whichever bits define it"
        assert p42["neighbours"] == 2, p42
        if name in C.SELECT:
            assert p42["cnt"] == 2 * C.SELECT[name][1]
    if name == "padded":
        assert C.slice_properties(c, R)["padded"] == [3, 4, 5, 6, 7]
    if name == "all-tied":
        assert p42["cnt"] == 2 * c.m


@pytest.mark.parametrize("name", SELECT_NAMES)
def test_gathered_model_and_its_faults(name):
    c = C.select_case(name)
    keys = SC.oracle_keys(c)
    R = C.SELECT_RANKS
    buf = C.gathered(keys, c.ii, c.m, R)
    assert buf.size == 2 * R * -(-c.m // R) and np.isinf(buf).sum() == buf.size - 2 * c.m
    med = S.lower_median(keys)
    m_local = int(np.diff(C.bounds(c.m, R)).min())
    assert S.gathered_model(buf, c.m, m_local) == med
    if name == "padded":
        assert S.gathered_model(buf, c.m, m_local, faults=("rank_from_count_all",)) != med
    got = S.gathered_model(buf, c.m, m_local, faults=("truncated_list_ranked",))
    if C.SELECT_BRANCH[name] == "overflow-short":
        assert got != med, "a truncated list ranked by counting gives another key (or none)"
    else:
        assert got == med, "the fault touches overflowed lists of <= 1024 keys only"


# ------------------------------------------------------------------------------------------------ the LM loop
def test_rejecting_windows_reject():
    for conf, accepted in ((2.2, True), (3.0, False)):
        c = C.rejecting(conf)
        it, init, lam = C.REJECT_CALL
        dbg = {}
        ntr = O.ba_iteration(it, c.states, c.cumrot, c.uv, c.xyz, c.ii, c.t, c.K, c.conf, lam, initialize=init, debug=dbg)[3]
        res = [t["residual"] for t in dbg["trials"]]
        assert ntr == C.REJECT_TRIALS[conf] and all(r >= dbg["init_residual"] for r in res[:-1]), (conf, ntr, res, dbg["init_residual"])
        assert (res[-1] < 0.97 * dbg["init_residual"]) == accepted and (accepted or res[-1] > 1.03 * dbg["init_residual"]), (conf, res)


@pytest.mark.parametrize("call", list(C.CALLS))
def test_plain_windows_accept_their_first_trial(call):
    for c in [C.slices()] + [C.head(r + 1) for r in C.SLICE_RANKS[1:]]:
        dbg, ntr = oracle_call(c, call)
        assert ntr == 1 and dbg["trials"][0]["residual"] < dbg["init_residual"], (c.name, call, ntr)


# ------------------------------------------------------------------------------------------------ partials and their reduction
def _oracle_parts(c, ranks, it, faults=()):
    med = S.lower_median(SC.oracle_keys(c))
    return med, [C.oracle_partial(c, C.rank_rows(c, ranks, r), med, it, faults) for r in range(ranks)]


@pytest.mark.parametrize("call", list(C.CALLS))
def test_oracle_partials_pass_and_a_missing_trip_fails(call):
    it = C.CALLS[call][0]
    for c, ranks in ((C.slices(), 8), (C.head(4), 3), (C.chain(), C.CHAIN_RANKS)):
        med, parts = _oracle_parts(c, ranks, it)
        for r, (part, est, Jg) in enumerate(parts):
            rows = C.rank_rows(c, ranks, r)
            bad, figs = C.check_partial(c, rows, part, est, Jg, med, it, -(-(rows.stop - rows.start) // 256), f"{c.name} rank {r}")
            assert not bad, bad
    c = C.chain()
    med, parts = _oracle_parts(c, C.CHAIN_RANKS, it, faults=("second_trip_missing",))
    caught = 0
    for r, (part, est, Jg) in enumerate(parts):
        rows = C.rank_rows(c, C.CHAIN_RANKS, r)
        bad, _f = C.check_partial(c, rows, part, est, Jg, med, it, -(-(rows.stop - rows.start) // 256), f"rank {r}")
        caught += bool(bad)
    assert caught == C.CHAIN_RANKS, "every rank has rows on poses behind the first trip"


def test_reduction_is_rank_ordered():
    c = C.slices()
    _med, parts = _oracle_parts(c, 3, C.IT_FULL)
    parts = [p[0] for p in parts]
    H, b = C.fetched_expected(parts, c.n)
    Hr, br = C.fetched_expected(parts, c.n, faults=("reverse_rank_order",))
    assert not (np.array_equal(H, Hr) and np.array_equal(b, br)), "three terms added the other way round round differently somewhere"
    assert np.allclose(H, Hr, rtol=1e-14, atol=0) and np.array_equal(H, np.swapaxes(H, 1, 2))
    Hraw, braw, wmax, sa = C.reduce_expected(parts, c.n)
    assert wmax == max(p[27 * c.n] for p in parts) and sa == (parts[0][-1] + parts[1][-1]) + parts[2][-1]


def test_device_order_sums():
    rng = np.random.default_rng(5)
    v = rng.uniform(0, 1, 64)
    assert abs(C._wave_sum(v) - v.sum()) < 1e-13 and C._wave_sum(np.arange(64.0)) == 2016.0
    rp = rng.normal(0, 1, (16, 7))
    ref = np.abs(rp).sum() * 1e3
    assert abs(C.sum_pred_model(rp, 1e6) - ref) < 1e-10 * ref
    init, trial = C.decide_expected([np.array([0.0] * 27 * 2 + [1.0, 3.0]), np.array([0.0] * 27 * 2 + [2.0, 5.0])], [(2.0, 1.0), (4.0, 1.0)], 2, 10,
                                    False, 6.0)
    assert init == (8.0 + 6.0) / 27.0 and trial == 7.0 / 27.0
