"""tests/trial_reference.py and tests/trial_cases.py without a GPU: the fp64 NumPy oracle's figures on every case (the bars of
tests/test_gpu_trial_paths.py come from them), the conditions on the cases, the restated device constants, and planted faults that
each check must reject.

The oracle's largest figure per group of cases, phase and quantity, in units of 2^-53 (``ORACLE``; both geometries of the pose-chain
slots, the larger one): no figure is above 4.01 (the retraction of mixed[30]), so every bar of the GPU test is the floor, 16 x 2^-53, or 16.04.  A case on which the oracle
does not accept its first trial at least 1 % below the initial residual fails here -- on the GPU side nothing would be carried and
the checks of the carried data would have nothing to look at."""
import numpy as np
import pytest

import dynamics_reference as R
import trial_cases as C
import trial_reference as T

QUANTITIES = ("retract", "step_fwd", "last_hessian", "part_obs", "part_next", "part_dyn", "part_long", "mean")
# (group, landmark-only) -> the oracle's largest figure per quantity, measured here on the CPU, rounded up to 0.01
ORACLE = {
    ('seams16', True): {'retract': 2.87, 'step_fwd': 0.84, 'last_hessian': 0.01, 'part_obs': 2.3, 'part_next': 1.5, 'part_dyn': 0.01, 'part_long': 0.01, 'mean': 1.07},
    ('seams16', False): {'retract': 4.01, 'last_hessian': 1.22, 'part_obs': 2.74, 'part_next': 2.02, 'part_dyn': 1.44, 'part_long': 0.01, 'mean': 0.29},
    ('seams256', True): {'retract': 3.81, 'step_fwd': 1.0, 'last_hessian': 0.01, 'part_obs': 1.74, 'part_next': 1.15, 'part_dyn': 0.01, 'part_long': 0.01, 'mean': 0.77},
    ('seams256', False): {'retract': 3.32, 'last_hessian': 1.0, 'part_obs': 0.97, 'part_next': 1.26, 'part_dyn': 0.47, 'part_long': 0.01, 'mean': 0.07},
    ('leaders', True): {'retract': 3.76, 'step_fwd': 2.08, 'last_hessian': 0.01, 'part_obs': 1.34, 'part_next': 1.25, 'part_dyn': 0.01, 'part_long': 0.01, 'mean': 0.65},
    ('leaders', False): {'retract': 3.93, 'last_hessian': 1.33, 'part_obs': 1.11, 'part_next': 1.09, 'part_dyn': 0.96, 'part_long': 0.01, 'mean': 0.2},
    ('tiles', True): {'retract': 3.4, 'step_fwd': 0.91, 'last_hessian': 0.51, 'part_obs': 1.61, 'part_next': 1.73, 'part_dyn': 0.01, 'part_long': 0.01, 'mean': 2.12},
    ('tiles', False): {'retract': 3.83, 'last_hessian': 1.2, 'part_obs': 1.7, 'part_next': 1.3, 'part_dyn': 0.79, 'part_long': 0.01, 'mean': 0.29},
    ('long', True): {'retract': 3.35, 'step_fwd': 0.58, 'last_hessian': 0.01, 'part_obs': 1.86, 'part_next': 0.19, 'part_dyn': 0.01, 'part_long': 0.01, 'mean': 0.2},
    ('long', False): {'retract': 2.86, 'last_hessian': 1.25, 'part_obs': 1.0, 'part_next': 0.18, 'part_dyn': 0.3, 'part_long': 0.98, 'mean': 0.13},
    ('BA_reg', True): {'retract': 3.5, 'step_fwd': 0.91, 'last_hessian': 0.36, 'part_obs': 2.3, 'part_next': 1.41, 'part_dyn': 0.01, 'part_long': 0.01, 'mean': 1.63},
    ('BA_reg', False): {'retract': 3.78, 'last_hessian': 2.14, 'part_obs': 1.52, 'part_next': 1.34, 'part_dyn': 1.17, 'part_long': 0.01, 'mean': 0.25},
}
_LEVELS = {}


def levels(s, init, lanes16):
    key = (s.name, init, lanes16)
    if key not in _LEVELS:
        _LEVELS[key] = T.oracle_levels(s.case, C.IT_INIT if init else C.IT, C.LAM_INIT if init else C.LAM, init, s.n_max, s.m_max, lanes16,
                                       reg=s.reg)
    return _LEVELS[key]


@pytest.mark.parametrize("init", [True, False], ids=["landmark-only", "full"])
@pytest.mark.parametrize("group", list(C.GROUPS))
def test_oracle_figures_and_case_conditions(group, init):
    """``oracle_levels`` asserts the conditions (first trial accepted with a margin, no figure above 1024 units, nothing where nothing
    is summed); the figures are the recorded ones."""
    got = {}
    for s in C.group(group):
        for lanes16 in (True, False):
            u = levels(s, init, lanes16).units
            for q in QUANTITIES:
                if q in u:
                    got[q] = max(got.get(q, 0.0), u[q])
    print(f"ORACLE ({group!r}, {init}): " + repr({q: round(v + 0.005, 2) for q, v in got.items()}))
    want = ORACLE[(group, init)]
    assert set(got) == set(want)
    for q, v in got.items():
        assert v <= want[q] + 1e-9, f"{group} {q}: the oracle stands at {v:.3f} units, recorded {want[q]}"
        assert 4 * v < R.K_FLOOR + 0.1, f"{group} {q}: the bar of this quantity is no longer (about) the floor"


def test_every_seam_of_the_issue_is_a_case():
    specs = C.all_specs()
    n16 = {s.case.n for s in C.group("seams16") if s.n_max == s.case.n}
    assert n16 == {2, 15, 16, 17, 30, 31, 32, 46}
    assert {(s.case.n, s.n_max) for s in C.group("seams16") if s.n_max != s.case.n} == {(16, 31), (16, 129)}
    assert {s.case.n for s in C.group("seams256")} == {255, 256, 257}
    assert {-(-s.case.m // 256) for s in C.group("tiles")} == {1, 2, 3, 4, 5, 8, 9}
    assert {0, 1, 255} <= {s.case.m % 256 for s in C.group("tiles")}
    one = C.one_row_each()
    assert one.n == 300 and np.array_equal(np.sort(one.ii), np.arange(300))
    h = C.holes()
    cnt = np.bincount(h.ii, minlength=h.n)
    assert cnt[0] == 0 and cnt[-1] == 0 and (cnt == 0).sum() >= 10
    assert any(s.reg for s in specs) and any(T.chain_terms(s.case.states, s.case.t, s.case.cumrot, 1.0, False)["long"].any() for s in C.group("long"))
    assert all(s.case.n <= 300 and s.case.m <= 6000 for s in specs)
    wins, n_max, m_max = C.ragged()
    assert min(w.m for w in wins) < 256 and max(w.m for w in wins) == m_max and max(w.n for w in wins) == n_max


# ------------------------------------------------------------------------------------------------ device constants
def _bits(x):
    return int(T.f64_bits([x])[0])


def test_warm_bins_restate_the_device_functions():
    lo = T.warm_range_start(_bits(1.0), 44)                 # 7 binades, 4 down: [1 / 16, 8)
    assert lo == _bits(1.0 / 16)
    assert T.warm_range_start(_bits(1.0), 43) == _bits(0.25)        # 3 binades, 2 down
    assert T.warm_range_start(_bits(1.0), 46) == _bits(2.0 ** -16)  # 31 binades, 16 down
    assert T.warm_range_start(0, 44) == 2 ** 64 - 1 and T.warm_range_start(_bits(np.inf), 44) == 2 ** 64 - 1
    assert T.warm_range_start(_bits(2.0 ** -1019), 44) == 2 ** 64 - 1      # exponent field 4 <= down
    keys = np.array([0.0, np.nextafter(1.0 / 16, 0), 1.0 / 16, 1.0 / 16 * (1 + 2.0 ** -8), 1.0, np.nextafter(8.0, 0) / 1.0, 7.99, 8.0, 1e9])
    got = T.warm_bin(T.f64_bits(keys), lo, 44)
    # 256 bins per binade: 1 sits 4 binades up (bin 1025), 8 seven binades up (bin 1793)
    assert list(got[:5]) == [0, 0, 1, 2, 1025]
    assert got[5] == 7 * 256 and got[7] == 1 + 7 * 256 and got[8] == 2047 and 1 + 6 * 256 <= got[6] <= 7 * 256
    # the 2046 bins end 254 bins into the eighth binade: 15.9 is in the last but one, 15.95 above the range
    assert list(T.warm_bin(T.f64_bits(np.array([15.9, 15.95, 16.0])), lo, 44)) == [2045, 2047, 2047]
    assert np.all(T.warm_bin(T.f64_bits(keys), 2 ** 64 - 1, 44) == 0)
    assert list(T.exp_digit(T.f64_bits(np.array([0.0, 1.0, 2.0, 4.0, 2.0 ** -1022])))) == [0, 511, 512, 512, 0]


# ------------------------------------------------------------------------------------------------ planted faults
def _device_like(s, lanes16, faults=(), weight=None):
    """What a fetch would hand out if the kernel summed as the reference does (``faults``: as it would with that mistake), fp64."""
    lv = levels(s, False, lanes16)
    o, c = lv.oracle, s.case
    tr = o["dbg"]["trials"][0]
    prior = c.prior() if s.reg else None
    ch = T.chain_terms(o["out"], c.t, c.cumrot, o["sigma"], False, False, prior)
    nl = int(ch["long"].sum())
    w = o["dbg"]["w"] if weight is None else weight
    good = T.slot_sums(c.uv, tr["est"], o["dbg"]["w"], c.ii, ch, s.n_max, s.m_max, lanes16, nl)
    made = T.slot_sums(c.uv, tr["est"], w, c.ii, ch, s.n_max, s.m_max, lanes16, nl, faults)
    pt = np.concatenate([made["obs"][0], made["dyn"][0], made["long"][0], np.zeros(3)]).astype(np.float64)
    return lv, good, pt, made["raw"][0].astype(np.float64), nl


def _verdict(s, lanes16, faults=(), weight=None):
    lv, good, pt, pn, nl = _device_like(s, lanes16, faults, weight)
    exact = []
    figs = T.slot_figures(good, pt, pn, nl, exact)
    mean, den = T.trial_mean(good, s.case.n, s.case.m, False, s.reg)
    no, nd = T.geometry(s.n_max, s.m_max, lanes16)
    per = 2 * s.case.m + 7 * (s.case.n - 1) + (7 * s.case.n if s.reg else 0)
    figs["mean"] = R.sums_figure((pt.sum() + (100.0 * s.case.n if s.reg else 0.0)) / per, mean, den)
    return R.judge(lv, figs, exact)


def _spec(group, name):
    return next(s for s in C.group(group) if s.name == name)


def test_the_reference_passes_its_own_sums():
    for s, lanes16 in ((_spec("BA_reg", "mixed[31] reg"), True), (_spec("tiles", "tiles[1025]"), False), (_spec("long", "long31[65]"), True)):
        v = _verdict(s, lanes16)
        assert v.ok and max(v.units.values()) < 2, (s.name, v.failures, v.units)


def test_a_dropped_16th_pose_edge_is_rejected():
    s = _spec("BA_reg", "mixed[16] reg")
    v = _verdict(s, True, ("drop_16th_edge",))
    assert v.units["part_dyn"] > v.bars["part_dyn"] and v.where["part_dyn"][0] == 0, v.units


def test_a_dropped_prior_of_the_last_pose_is_rejected():
    for name in ("mixed[31] reg", "mixed[46] reg", "mixed[16] reg"):       # n_max - 1 a multiple of 15: the 16th lane group of the last block
        s = _spec("BA_reg", name)
        assert (s.n_max - 1) % 15 == 0
        v = _verdict(s, True, ("drop_last_prior",))
        assert v.units["part_dyn"] > v.bars["part_dyn"] and v.where["part_dyn"][0] == T.geometry(s.n_max, s.m_max, True)[1] - 1, (name, v.units)


def test_a_boundary_row_in_both_tiles_is_rejected():
    v = _verdict(_spec("tiles", "tiles[1025]"), False, ("boundary_row_twice",))
    assert v.units["part_obs"] > v.bars["part_obs"] and v.units["part_next"] > v.bars["part_next"], v.units


def test_a_partial_written_one_slot_late_is_rejected():
    v = _verdict(_spec("tiles", "tiles[1025]"), False, ("tile_one_slot_late",))
    assert v.units["part_obs"] > v.bars["part_obs"] and v.units["part_next"] > v.bars["part_next"], v.units
    assert v.units["mean"] < v.bars["mean"], "the total does not see a shifted slot: only the slots do"


def test_weights_of_the_other_parity_are_rejected():
    """The next call's weights (formed at the trial states) where the trial's sums take this call's."""
    from oracle import ba_oracle as O
    s = _spec("tiles", "tiles[1025]")
    o, c = levels(s, False, False).oracle, s.case
    w_next = O.robust_weights(c.uv - o["dbg"]["trials"][0]["est"], C.IT, c.conf)[0]
    v = _verdict(s, False, weight=w_next)
    assert v.units["part_obs"] > v.bars["part_obs"] and v.units["part_next"] < 2, v.units


def _carried(s, shift=44):
    o, c = levels(s, False, False).oracle, s.case
    keys = T.expected_keys(c.uv, o["dbg"]["trials"][0]["est"])
    lo = T.warm_range_start(_bits(float(o["dbg"]["c_obs"])), shift)
    bins = T.warm_bin(T.f64_bits(keys.reshape(-1)), lo, shift)
    hist = np.bincount(bins, minlength=2048).astype(np.uint64)
    cap = 8
    bk = np.zeros((2048, cap))
    fill = np.zeros(2048, dtype=np.int64)
    for k, b in zip(keys.reshape(-1), bins):
        if 1 <= b <= 2046 and fill[b] < cap:
            bk[b, fill[b]] = k
        fill[b] += 1
    return keys, lo, shift, hist, bk, cap, float(o["dbg"]["c_obs"])


def test_carried_data_checks_pass_and_reject():
    s = _spec("tiles", "tiles[1025]")
    keys, lo, shift, hist, bk, cap, c_obs = _carried(s)
    est = levels(s, False, False).oracle["dbg"]["trials"][0]["est"]
    assert (hist[1:2047] > cap).any() and ((hist[1:2047] > 1) & (hist[1:2047] <= cap)).any()
    assert not T.check_keys(keys, s.case.uv, est)
    assert not T.check_hist(keys, 2, lo, shift, hist, c_obs)
    assert not T.check_buckets(keys, lo, shift, hist, bk, cap)
    e1 = np.bincount(T.exp_digit(T.f64_bits(keys.reshape(-1))), minlength=1024)
    assert not T.check_hist(keys, 1, 0, 0, e1, sel_rank=(keys.size - 1) // 2)
    assert T.check_hist(keys, 1, 0, 0, e1, sel_rank=keys.size // 2)
    # one bit of one key
    k2 = keys.copy()
    k2[7, 1] = np.nextafter(k2[7, 1], np.inf)
    assert T.check_keys(k2, s.case.uv, est)
    # a key counted in the neighbouring bin (no bin near the median: the next median would still come out exact)
    b = int(np.nonzero(hist[1:2046])[0][3]) + 1
    h2 = hist.copy()
    h2[b] -= 1
    h2[b + 1] += 1
    assert T.check_hist(keys, 2, lo, shift, h2, c_obs) and int(h2.sum()) == keys.size
    assert T.check_buckets(keys, lo, shift, h2, bk, cap)
    # a bucket slot written twice: one key of the bin duplicated over another
    b = next(b for b in range(1, 2047) if 1 < hist[b] <= cap and bk[b, 0] != bk[b, 1])
    bk2 = bk.copy()
    bk2[b, 1] = bk2[b, 0]
    assert T.check_buckets(keys, lo, shift, hist, bk2, cap)
    # ... and in a full bucket, where only a sub-multiset is asked for
    b = int(np.nonzero(hist[1:2047] > cap)[0][0]) + 1
    bk3 = bk.copy()
    src = bk3[b, 0]
    if np.count_nonzero(keys.reshape(-1) == src) == 1:
        bk3[b, 1] = src
        assert T.check_buckets(keys, lo, shift, hist, bk3, cap)
    # a warm range that does not belong to the call's median
    assert T.check_hist(keys, 2, lo, shift, hist, c_obs * 2)
