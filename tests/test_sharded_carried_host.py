"""The model of ``k_sh_front`` and the exchange pattern of tests/test_gpu_sharded_carried.py on hand-made data (no GPU): every miss reason,
both boundary twins, the pose-chain part taken from slot 0, the summation order, the conditions on the windows, and planted faults
showing that a wrong layer is seen."""
import numpy as np
import pytest

import sharded_carried_cases as K
import sharded_stage_cases as C
import trial_reference as TR

NBO, STRIDE, NCHAIN = 2, 2 + 3 + 64, 3
LO = 0x3FF0000000000000


def slot(hist, nxt=(0.0, 0.0), trial=(0.0, 0.0), chain=(0.0, 0.0, 0.0)):
    pt = np.zeros(STRIDE)
    pt[:NBO], pt[NBO:NBO + NCHAIN] = trial, chain
    return K.pack_a(hist, np.asarray(nxt, dtype=np.float64), pt)


def hists(per_rank_in_bin, b=1000, below=None, total=None):
    """R histograms with ``per_rank_in_bin`` keys in bin ``b`` and as many keys below the bin as above it (rank 0 holds them)."""
    R = len(per_rank_in_bin)
    hs = [np.zeros(K.SEL_BINS, dtype=np.uint32) for _ in range(R)]
    for r, k in enumerate(per_rank_in_bin):
        hs[r][b] = k
    n_in = sum(per_rank_in_bin)
    side = 10 if below is None else below
    hs[0][max(b - 1, 0) if b > 0 else 0] += side if b > 0 else 0
    hs[-1][min(b + 1, K.SEL_BINS - 1)] += (side if total is None else total - side - n_in) + (n_in % 2)
    m_total = sum(int(h.sum()) for h in hs) // 2
    return hs, m_total


def resolve(per, cap=256, b=1000, forced=False, lo=LO, faults=()):
    hs, m_total = hists(per, b)
    return K.front_resolve([slot(h) for h in hs], m_total, cap, lo, forced, faults), m_total


def test_the_bin_and_the_rank_inside_it():
    d, m_total = resolve((4, 3, 2))
    assert d["bin"] == 1000 and d["in_bin"] == 9 and d["hit"] and d["reason"] is None
    assert d["rank"] == (2 * m_total - 1) // 2 - 10 and 0 <= d["rank"] < 9
    assert [int(h[1000]) for h in d["own"]] == [4, 3, 2]


@pytest.mark.parametrize("per, cap, reason", [((9, 8, 1), 8, "overflow"), ((8, 8, 4), 8, None), ((205,) * 5, 256, "long"),
                                               ((205, 205, 205, 205, 204), 256, None), ((256,) * 4, 256, None), ((257, 1, 1), 256, "overflow")])
def test_miss_reasons_and_boundary_twins(per, cap, reason):
    d, _m = resolve(per, cap)
    assert d["reason"] == reason and d["hit"] == (reason is None), d
    if reason == "overflow":
        assert d["over"] == [0], "one rank alone overflowed"


def test_leaving_forced_and_no_range():
    for b in (0, 2047):             # (60 keys in the bin, 10 on its one neighbour: the median lies in the bin)
        d = resolve((30, 30), b=b)[0]
        assert d["bin"] == b and d["reason"] == "leaving", d
    assert resolve((3, 3), b=1)[0]["hit"] and resolve((3, 3), b=2046)[0]["hit"]
    assert resolve((3, 3), lo=(1 << 64) - 1)[0]["reason"] == "leaving"
    d = resolve((3, 3), forced=True)[0]
    assert d["reason"] == "forced" and d["reasons"] == ["forced"]


def test_planted_faults_in_the_resolve_step():
    good, _m = resolve((4, 3, 20))
    assert resolve((4, 3, 20), faults=("drop_last_rank",))[0]["in_bin"] != good["in_bin"], "a histogram summed over R - 1 ranks is seen"
    assert resolve((8, 8, 4), 8)[0]["hit"] and not resolve((8, 8, 4), 8, faults=("cap_ge",))[0]["hit"], "> against >= on the cap is seen"


def test_planted_faults_in_bucket_median_and_key_exchange():
    """The comparisons ``judge`` makes for layers c and d (``check_bucket``, ``check_median``, ``check_key_exchange``) on faulted data."""
    rng = np.random.default_rng(5)
    keys = np.abs(rng.normal(2.7, 0.004, (40, 2)))
    lo = TR.warm_range_start(int(TR.f64_bits([2.7])[0]), K.SHIFT)
    h = K.own_hist(keys, lo)
    assert int(h.sum()) == 80
    b = int(np.argmax(h))
    assert h[b] > 2 and h[b + 1] > 0
    mine = K.expected_bucket(keys, lo, b).view(np.float64)
    good = np.concatenate([[float(h[b])], rng.permutation(mine), np.zeros(3)])
    assert K.check_bucket(good, keys, lo, b, h[b]) == []
    nb = K.expected_bucket(keys, lo, b + 1).view(np.float64)
    assert K.check_bucket(np.concatenate([[float(nb.size)], nb]), keys, lo, b, h[b]), "a bucket from the neighbouring bin"
    assert K.check_bucket(np.concatenate([[float(h[b])], mine[:-1], mine[:1]]), keys, lo, b, h[b]), "a key twice, one missing"
    assert K.check_bucket(np.concatenate([[float(h[b] - 1)], mine[:-1]]), keys, lo, b, h[b]), "a truncated bucket"
    assert K.check_bucket(good, keys, lo, b, h[b] + 1), "a count that is not the histogram word"
    ranks = [keys[:13], keys[13:30], keys[30:]]
    allk = np.sort(keys.reshape(-1))
    assert K.check_median(allk[39], ranks) == []
    assert K.check_median(allk[40], ranks) and K.check_median(allk[38], ranks), "a median one rank off"
    assert K.check_median(float(np.sort(ranks[0].reshape(-1))[12]), ranks), "a rank's local median"
    ii = np.array([3, 1, 2, 1, 0])
    k5 = keys[:5]
    sent = np.concatenate([k5[np.argsort(ii, kind="stable")].reshape(-1), np.full(4, np.inf)])
    assert K.check_key_exchange(sent, k5, ii, 7) == []
    assert K.check_key_exchange(np.concatenate([k5.reshape(-1), np.full(4, np.inf)]), k5, ii, 7), "keys in input order"
    stale = sent.copy()
    stale[-1] = 2.7
    assert K.check_key_exchange(stale, k5, ii, 7), "an old key left in the padding"


def test_a_partial_at_the_local_median_is_seen():
    """Layer e: ``check_partial`` at the global median refuses the oracle's partial of a rank formed at that rank's own median."""
    import select_cases as SC
    import select_reference as S
    c = C.slices()
    keys = SC.oracle_keys(c)
    rows = C.rank_rows(c, 3, 0)
    med, local = S.lower_median(keys), S.lower_median(keys[rows])
    assert med != local
    good, est, Jg = C.oracle_partial(c, rows, med, 0)
    assert C.check_partial(c, rows, good, est, Jg, med, 0, 1, "rank 0", sum_slot=False)[0] == []
    wrong = C.oracle_partial(c, rows, local, 0)[0]
    assert C.check_partial(c, rows, wrong, est, Jg, med, 0, 1, "rank 0", sum_slot=False)[0]


@pytest.mark.parametrize("name", list(K.BAND))
def test_conditions_on_the_band_windows(name):
    """With the oracle's keys: one accepted trial, the first median is the pivot, the second call's median lies in the bin that ends
    there, and that bin holds the band: so many keys per rank as the case says (which rank overflows, how long the bin is)."""
    R, cap, m_r, per = K.BAND[name]
    q = K.band_conditions(name)
    assert q["trials"] == 1 and q["m"] == R * m_r and abs(q["med0"] - K.PIVOT) < 1e-9
    assert q["bin"] == 1024 and q["per_rank"] == list(per) and q["in_bin"] == sum(per)
    limit = cap or 256
    assert [r for r in range(R) if per[r] > limit] == ([0] if name == "overflow-one-rank" else [])
    assert (sum(per) > K.LIST_MAX) == (name == "long-bin") and max(per) == (10 if name == "overflow-one-rank" else limit if cap else 205)
    reason = "overflow" if any(v > limit for v in per) else ("long" if sum(per) > K.LIST_MAX else None)
    assert reason == K.BAND_REASON[name]


def test_conditions_on_the_leaving_window():
    q = K.band_conditions("leaving")
    assert q["trials"] == 1 and q["m"] <= 2000 and q["med1"] < q["med0"] / 16 and q["bin"] == 0


def test_trial_counts_of_the_rejecting_windows():
    from oracle import ba_oracle as O
    for conf, want in C.REJECT_TRIALS.items():
        c = C.rejecting(conf)
        it, init, lam = C.REJECT_CALL
        assert O.ba_iteration(it, c.states, c.cumrot, c.uv, c.xyz, c.ii, c.t, c.K, c.conf, lam, initialize=init)[3] == want
        assert K.lam0_of(f"rejecting-{conf:g}/step") == lam


def test_sums_order_and_slot_zero():
    rng = np.random.default_rng(7)
    h = np.zeros(K.SEL_BINS, dtype=np.uint32)
    slots = [slot(h, rng.uniform(1, 2, 2) * 1e3, rng.uniform(1, 2, 2) * 1e3, rng.uniform(1, 2, 3) * (q + 1)) for q in range(3)]
    s_next, s_trial = K.front_sums(slots, NBO, NCHAIN)
    # by hand: thread t holds block t of every rank (rank order), then the chain block t of slot 0; lanes 0 .. 2 of wave 0
    t = [0.0, 0.0, 0.0]
    nx = [0.0, 0.0]
    for q in range(3):
        for b in range(NBO):
            t[b] = t[b] + slots[q][1024 + NBO + b]
            nx[b] = nx[b] + slots[q][1024 + b]
    for b in range(NCHAIN):
        t[b] = t[b] + slots[0][1024 + 2 * NBO + b]
    lanes = np.zeros(64)
    lanes[:3] = t
    assert s_trial == C._wave_sum(lanes) and s_next == nx[0] + nx[1]
    assert K.front_sums(slots, NBO, NCHAIN, ("chain_from_every_rank",))[1] != s_trial, "the pose-chain part added R times is seen"
    other = [slots[1], slots[0], slots[2]]
    assert K.front_sums(other, NBO, NCHAIN)[1] != s_trial, "the pose-chain part comes from slot 0"
    i0, t0 = K.residuals(s_next, 0.25, s_trial, 17, 91, False)
    assert i0 == (s_next + 0.25) / (2.0 * 91 + 7.0 * 16) and t0 == s_trial / (2.0 * 91 + 7.0 * 16)
    assert K.residuals(s_next, 0.25, s_trial, 17, 91, True)[0] == s_next / (2.0 * 91 + 6.0 * 16)
    d = K.front_model(slots, 91, 256, LO, NBO, NCHAIN, 17, False, 1234.5, 0.25)
    assert d["sum_in"] == s_next and (d["init_residual"], d["trial_residual"]) == K.residuals(1234.5, 0.25, s_trial, 17, 91, False)


def test_pattern_and_lengths():
    assert K.len_a(1, 67) == (1024 + 1 + 67 + 3) & ~3 and K.len_b(256) == 260 and K.len_b(8) == 12
    lenA, lenB = K.len_a(1, 67), K.len_b(256)
    assert K.pattern(True, False, False, 1, lenA, lenB, 17, 31) == [lenB, 461, lenA]
    assert K.pattern(False, False, False, 1, lenA, lenB, 17, 31) == [62, 461, lenA]
    assert K.pattern(True, True, False, 1, lenA, lenB, 17, 31) == [lenB, 461, lenA, 62, 461, lenA]
    assert K.pattern(True, False, True, 5, lenA, lenB, 17, 31) == [lenB, 461, lenA, 2, 2, 2, 2, 2, lenA]
    # a handle that quietly takes the round-3 protocol gathers keys, C and 2 doubles per trial: no pattern above matches it
    assert [62, 461, 2] not in [K.pattern(c, m, s, 1, lenA, lenB, 17, 31) for c in (0, 1) for m in (0, 1) for s in (0, 1)]


def test_split_and_pack_round_trip():
    h = np.arange(K.SEL_BINS, dtype=np.uint32)
    a = slot(h, (1.0, 2.0), (3.0, 4.0), (5.0, 6.0, 7.0))
    hh, pn, pt = K.split_a(a, NBO, STRIDE)
    assert np.array_equal(hh, h) and pn.tolist() == [1.0, 2.0] and pt[:5].tolist() == [3.0, 4.0, 5.0, 6.0, 7.0] and a.size % 4 == 0


@pytest.mark.parametrize("world", [1, 2, 3])
def test_conditions_on_the_windows(world):
    c = C.slices()
    assert c.m == 91 and (world == 1 or c.m % world != 0)
    for resplit in (False, True):
        b = K.split_bounds(c.m, world, resplit and world > 1)
        assert b[0] == 0 and b[-1] == c.m and np.all(np.diff(b) <= -(-c.m // world)) and np.all(np.diff(b) >= 1)
    assert C.head(world + 1).m == world + 1
    s = K.scenarios(world)
    assert all(K.case_of(name, world)[0].m >= world for name in s) and ("slices/reupload" in s) == (world > 1)
    assert set(K.scenarios(5)) == {"long-bin/step", "long-twin/step"} and max(v[0] for v in K.BAND.values()) <= K.MAX_WORLD
    if world == 3:
        assert {"rejecting-2.2/step", "rejecting-3/chain", "overflow-one-rank/step", "overflow-twin/step", "leaving/step"} <= set(s) and K.lam0_of("rejecting-3/step") == C.REJECT_CALL[2]
