"""vba_snoop_scaled: data snooping with one critical value per window, quantile * s0 of the window's own fit, formed on the device
behind one covariance step.  The contract: per window the handle ends where vba_outlier_power, a host multiply and
vba_snoop(crit_used[w]) would leave a handle that holds only that window -- s0sq with the bits of vba_outlier_power's fit,
crit_used with the bits of the host product, mask and counts of vba_snoop at that value; the promise and the boundary behaviour of
vba_snoop; the two streaming drivers over the same rounds; the error returns.

Masks against the NumPy oracle are compared exactly only where the oracle reports no ambiguous pose (tests/snoop_oracle.py), a
property of the test's inputs; masks of the device against the device (alone and in a batch, one call and three) are bit exact by
contract."""
import functools

import numpy as np
import pytest

import power_oracle as PW
import snoop_oracle as S
import snoop_scaled_windows as SSW
import snoop_windows as SW
from query_windows import INITS, SMALL_LAMDA, _ba_args, _batch_engine, _engine, _scheduled, _small_windows, _win
from test_gpu_snoop import BARRED, _gap_crit, _zeroed

pytestmark = pytest.mark.gpu

PINS = dict(lanes=8, fusion=12, solver=(8, -1), mode="lat")       # (the settings of tests/test_gpu_batch_surface.py's bitwise comparison)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------ smallest shapes
def test_smallest_shapes_alone_and_in_a_batch():
    """A 2-pose window with 3 rows on pose 0; 17 poses (two blocks of the grid) with 1, 16, 17 and 33 rows on poses 0..3 in shuffled
    input order; a window with every confidence zero -- one ragged batch, iter 12, damped at SMALL_LAMDA, modes 0 and 1, min_rows 2
    and 16.  Per window: s0sq is vba_outlier_power's, crit_used the host product, mask and counts those of vba_snoop(crit_used)
    on an engine that holds the window alone."""
    wins = _small_windows()
    two, many, dead = wins
    big = _batch_engine(wins, chunk=0)
    ones = [_batch_engine([w], chunk=0, sizes=(big.n_max, big.m_max), mode=big.mode()[0]) for w in wins]
    _, wt, _ = big.reliability(12, damped=True)
    fit = big.outlier_power(12, damped=True)[5]
    assert (fit[:2, 4] > 0).all() and np.isnan(fit[2, 4])
    quantile = _gap_crit(np.concatenate([wt[k, :w.m] / np.sqrt(fit[k, 4]) for k, w in enumerate((two, many))]))
    nonempty = 0
    for mode in (0, 1):
        for min_rows in (2, 16):
            rej, counts, crit, s0sq, flags = big.snoop_scaled(12, quantile, mode=mode, min_rows=min_rows, damped=True)
            assert not (flags & BARRED).any()
            assert np.array_equal(_bits(s0sq[:2]), _bits(fit[:2, 4])) and np.array_equal(s0sq, fit[:, 4], equal_nan=True)
            assert np.array_equal(_bits(crit[:2]), _bits(np.float64(quantile) * np.sqrt(s0sq[:2])))
            assert np.isnan(crit[2]) and not rej[2].any() and list(counts[2]) == [0, 0]     # the window without weights
            for k, one in enumerate(ones[:2]):                                              # each window alone, the three-step form
                assert _bits(one.outlier_power(12, damped=True)[5][0, 4]) == _bits(s0sq[k])
                r1, c1, f1 = one.snoop(12, crit[k], mode=mode, min_rows=min_rows, damped=True)
                assert np.array_equal(r1[0], rej[k]) and list(c1[0]) == list(counts[k]) and f1[0] == flags[k], (k, mode, min_rows)
                nonempty += int(r1[0].any())
                one.snoop_restore()
            r3, c3, cr3, s3, _ = ones[2].snoop_scaled(12, quantile, mode=mode, min_rows=min_rows, damped=True)
            assert not r3.any() and list(c3[0]) == [0, 0] and np.isnan(cr3[0]) and np.isnan(s3[0])
            got, tot = big.rejected()
            assert np.array_equal(got, rej) and list(tot) == [int(c[1]) for c in counts]
            big.snoop_restore()
            assert not big.rejected()[0].any()
    assert nonempty > 0                                                                     # (not a comparison of empty masks only)
    big.close()
    for one in ones:
        one.close()


def test_smallest_shapes_against_the_oracle_alone():
    """The same shapes, nothing of the device in the reference: s0 of tests/power_oracle.py, wtest of tests/snoop_oracle.py, the
    mask of ``snoop_oracle.select`` at quantile * s0 -- after the oracle reports no ambiguous pose at that value (1 +- 1e-6)."""
    wins = _small_windows()
    two, many, _ = wins
    refs = []
    for w in (two, many):
        wt, wgt = S.at_states(w, w.states0, SMALL_LAMDA, it=12, damped=True)
        s0 = float(np.sqrt(PW.at_states(w, w.states0, SMALL_LAMDA, it=12, damped=True)[0]["fit"][4]))
        refs.append((wt, wgt, s0))
    quantile = _gap_crit(np.concatenate([wt / s0 for wt, _, s0 in refs]))
    big = _batch_engine(wins, chunk=0)
    for mode in (0, 1):
        for min_rows in (2, 16):
            rej, counts, crit, s0sq, _ = big.snoop_scaled(12, quantile, mode=mode, min_rows=min_rows, damped=True)
            for k, w in enumerate((two, many)):
                wt, wgt, s0 = refs[k]
                assert abs(np.sqrt(s0sq[k]) / s0 - 1.0) < 1e-6
                for f in (1.0 - 1e-6, 1.0, 1.0 + 1e-6):
                    assert S.ambiguous(wt, wgt, w.ii, w.n, quantile * s0 * f, mode, min_rows) == []
                want, _ = S.select(wt, wgt, w.ii, w.n, quantile * s0, mode, min_rows)
                assert np.array_equal(rej[k, :w.m], want) and list(counts[k]) == [int(want.sum())] * 2, (k, mode, min_rows)
            big.snoop_restore()
    big.close()


# ------------------------------------------------------------------------------------------------ per-window decisions, the promise
SIX = (list(range(14, 20)), [False] * 6)


@functools.lru_cache(maxsize=None)
def _two_windows():
    """C1 seeds 0 and 1 on one handle after 14 calls, window 1's detections inflated by 5 px of noise (the oracle gives s0 0.82 and
    3.8); one vba_snoop_scaled (mode 1), six more scheduled calls; and the fresh handle with those confidences zeroed."""
    import copy
    from vinsat_amd import od_pipe
    from vinsat_amd.engine import BAEngine
    wins = [_win("C1", seed=0), copy.copy(_win("C1", seed=1))]
    wins[1].landmarks_uv = wins[1].landmarks_uv + np.random.default_rng(7).normal(0.0, 5.0, wins[1].landmarks_uv.shape)
    ns, ms = [w.states_gt.shape[0] for w in wins], [w.ii.size for w in wins]

    def make(confs):
        eng = BAEngine(max(ns), max(ms), windows=2)
        for k, w in enumerate(wins):
            eng.upload_observations(w.landmarks_xyz, w.landmarks_uv, confs[k], w.ii, ns[k], window=k)
            eng.upload_window(w.intrinsics, w.cumrot_last, w.time_idx, window=k)
        return eng

    a = make([w.confidences for w in wins])
    for k, w in enumerate(wins):
        a.set_states(od_pipe.initial_guess(w), 1e-4, window=k)
    a.run_schedule(list(range(14)), INITS[:14])
    S0, L0, _, _, _ = a.get_states_all()
    _, wt, _ = a.reliability(13)
    fit = a.outlier_power(13)[5]
    quantile = float(np.percentile(wt[0, :ms[0]], 90) / np.sqrt(fit[0, 4]))
    rej, counts, crit, s0sq, _ = a.snoop_scaled(13, quantile, mode=1, min_rows=6)
    S1, L1, _, _, _ = a.get_states_all()
    a.run_schedule(*SIX)
    got = (a.get_states_all()[:2], a.reliability(19, pose_stats=True))
    a.close()
    b = make([_zeroed(w.confidences, rej[k, :ms[k]]) for k, w in enumerate(wins)])
    b.set_states_all(S0, L0)
    b.run_schedule(*SIX)
    ref = (b.get_states_all()[:2], b.reliability(19, pose_stats=True))
    b.close()
    return dict(wins=wins, ns=ns, ms=ms, wt=wt, fit=fit, quantile=quantile, rej=rej, counts=counts, crit=crit, s0sq=s0sq,
                before=(S0, L0), after=(S1, L1), got=got, ref=ref)


def test_windows_of_one_call_decide_against_their_own_critical_values():
    """The case one ``crit`` cannot serve: the two s0 differ by more than 2, so a w-test between the two critical values is a
    candidate in window 0 and none in window 1."""
    r = _two_windows()
    ms, wt, rej, crit = r["ms"], r["wt"], r["rej"], r["crit"]
    s0 = np.sqrt(r["s0sq"])
    assert np.array_equal(_bits(r["s0sq"]), _bits(r["fit"][:, 4])) and s0[1] > 2.0 * s0[0]
    assert crit[0] != crit[1] and np.array_equal(_bits(crit), _bits(np.float64(r["quantile"]) * s0))
    w0, w1 = wt[0, :ms[0]], wt[1, :ms[1]]
    between0 = (w0 > crit[0]) & (w0 < crit[1])
    assert (between0 & rej[0, :ms[0]]).any()                        # rejected in window 0 below window 1's critical value
    assert (w0[rej[0, :ms[0]]] > crit[0]).all() and (w1[rej[1, :ms[1]]] > crit[1]).all()
    between1 = (w1 > crit[0]) & (w1 < crit[1])
    assert between1.any() and not rej[1, :ms[1]][between1].any()    # and kept in window 1 above window 0's
    assert r["counts"][0, 0] == rej[0].sum() > 0 and r["counts"][1, 0] == rej[1].sum()


def test_promise_on_a_two_window_handle():
    """States and lamda untouched by the call; six scheduled calls and a reliability query later the handle has the bits of a
    fresh one uploaded with those confidences zeroed."""
    r = _two_windows()
    ns, ms, got, ref = r["ns"], r["ms"], r["got"], r["ref"]
    assert np.array_equal(r["before"][0], r["after"][0]) and np.array_equal(r["before"][1], r["after"][1])
    for k in range(2):
        assert np.array_equal(got[0][0][k, :ns[k]], ref[0][0][k, :ns[k]]) and got[0][1][k] == ref[0][1][k]
        for x, y, cnt in zip(got[1][:3], ref[1][:3], (ms[k], ms[k], ns[k])):
            assert np.array_equal(x[k, :cnt], y[k, :cnt], equal_nan=True)


def test_promise_on_a_one_window_latency_mode_handle():
    """Graph replay and pipelining live: the six-call schedule has run (and been captured as a graph) before the call and runs again
    behind it, and a speculated call of the pipelined loop is pending when it arrives."""
    win = _win("C1")
    n, m = win.states_gt.shape[0], win.ii.size
    a = _engine(win)
    assert a.mode()[0] == 1
    _scheduled(win, a, calls=14)
    a.run_schedule(*SIX)
    _, wt, _ = a.reliability(19)
    s0 = float(np.sqrt(a.outlier_power(19)[5][0, 4]))
    st, lam, _, _, _ = a.iterate_resident(19, False)
    rej, counts, crit, s0sq, flags = a.snoop_scaled(19, float(np.percentile(wt[0, :m], 90)) / s0, mode=1, min_rows=6)
    assert counts[0, 0] > 0 and counts[0, 0] == rej[0, :m].sum() and _bits(crit)[0] != 0
    s1, l1, _, _, _ = a.get_states()
    assert np.array_equal(s1, st) and l1 == lam                 # states and lamda untouched
    a.run_schedule(*SIX)
    got = (a.get_states()[:2], a.reliability(19, pose_stats=True))
    a.close()
    b = _engine(win)
    b.upload_observations(win.landmarks_xyz, win.landmarks_uv, _zeroed(win.confidences, rej[0, :m]), win.ii, n)
    b.set_states(st, lam)
    b.run_schedule(*SIX)
    ref = (b.get_states()[:2], b.reliability(19, pose_stats=True))
    b.close()
    assert np.array_equal(got[0][0], ref[0][0]) and got[0][1] == ref[0][1]
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(got[1], ref[1]))
    assert (got[1][1][0, :m][rej[0, :m]] == 0.0).all()          # a rejected row has weight zero: wtest 0


# ------------------------------------------------------------------------------------------------ nothing rejected, restore, upload
def test_a_clean_round_an_infinite_quantile_restore_and_upload_leave_the_bits_of_a_handle_that_never_snooped():
    win = _win("C1")
    n, m = win.states_gt.shape[0], win.ii.size

    def tail(eng):
        eng.run_schedule(*SIX)
        s, l, _, _, _ = eng.get_states()
        return s, l

    c = _engine(win)
    st, lam = _scheduled(win, c, calls=14)
    _, wt, _ = c.reliability(13)
    s0 = float(np.sqrt(c.outlier_power(13)[5][0, 4]))
    quantile = float(np.percentile(wt[0, :m], 90)) / s0
    ref = tail(c)
    c.close()
    # a finite quantile no row reaches, and +inf
    for q in (1e6, np.inf):
        b = _engine(win)
        _scheduled(win, b, calls=14)
        rej, counts, crit, s0sq, _ = b.snoop_scaled(13, q, mode=1, min_rows=0)
        assert not rej.any() and list(counts[0]) == [0, 0] and crit[0] == q * np.sqrt(s0sq[0]) and b.last_snoop_ms() > 0.0
        got = tail(b)
        assert np.array_equal(got[0], ref[0]) and got[1] == ref[1]
        b.close()
    # restore
    a = _engine(win)
    _scheduled(win, a, calls=14)
    rej, counts, _, _, _ = a.snoop_scaled(13, quantile, mode=1, min_rows=6)
    assert counts[0, 0] > 0
    a.snoop_restore(0)
    assert not a.rejected()[0].any() and a.rejected()[1][0] == 0
    got = tail(a)
    assert np.array_equal(got[0], ref[0]) and got[1] == ref[1]
    # after a restore the same call rejects the same rows; an upload clears the mask (and brings the confidences of the new rows)
    a.set_states(st, lam)
    rej2, counts2, _, _, _ = a.snoop_scaled(13, quantile, mode=1, min_rows=6)
    assert np.array_equal(rej2, rej) and list(counts2[0]) == list(counts[0])
    a.upload_observations(win.landmarks_xyz, win.landmarks_uv, win.confidences, win.ii, n)
    assert not a.rejected()[0].any() and a.rejected()[1][0] == 0
    a.set_states(st, lam)
    got = tail(a)
    assert np.array_equal(got[0], ref[0]) and got[1] == ref[1]
    a.close()


# ------------------------------------------------------------------------------------------------ the drivers
def _same_result(x, y):
    import torch
    return torch.equal(x[0], y[0]) and x[1] == y[1] and all(np.array_equal(np.atleast_1d(a), np.atleast_1d(b)) for a, b in zip(x[2], y[2]))


def test_the_batched_driver_against_the_sequential_one_and_ba_snoop_scaled_against_ba_snoop():
    """``streaming_batched(snoop_each=...)`` on [the planted C2 sequence, C1] against ``streaming_version(snoop=dict(scaled=True,
    ...))`` per sequence, two rounds of four calls with ``until="rounds"`` in both, equal handle settings: the same rejected rows,
    errors and time stamps, bit for bit.  Quantile 3.29, vetted on the CPU (tests/test_snoop_scaled_host.py): the oracle's loop
    rejects 67 and 26 rows of the C2 sequence (margins 1.7e-4, 4.1e-5) and 2 and 0 of C1 (2.8e-6, 2.0e-6), no pose ambiguous."""
    import torch
    from vinsat_amd import ba, od_pipe
    seqs = SSW.sequences()
    copies = lambda: [(d.copy(), o.copy()) for d, o in seqs]
    cfg = dict(crit=SSW.QUANTILE, rounds=SSW.ROUNDS, calls=SSW.CALLS, mode=SSW.MODE, min_rows=SSW.MIN_ROWS, until="rounds")
    ba.configure(**PINS)
    try:
        plain = od_pipe.streaming_batched(copies())
        ba.release()
        none = od_pipe.streaming_batched(copies(), snoop_each=None)
        ba.release()
        assert all(_same_result(x, y) for x, y in zip(plain, none))
        log = []
        got = od_pipe.streaming_batched(copies(), snoop_each=cfg, snoop_log=log)
        ba.release()
        assert [(r["round"], r["sequence"]) for r in log] == [(0, 0), (0, 1)]
        for k, (det, orb) in enumerate(seqs):
            own = []
            ref = od_pipe.streaming_version(det.copy(), orb.copy(), snoop=dict(cfg, scaled=True), snoop_log=own)
            ba.release()
            assert len(own) == 1 and np.array_equal(own[0], log[k]["rows"]), k
            assert own[0].size > 0, k
            assert _same_result(got[k], ref), k
        assert not _same_result(got[0], plain[0])                   # (the rejections changed the estimate)
        # one window through the module: the one-call form against ba.snoop's two queries
        _, _, win, _ = SW.planted()
        args = _ba_args(win)
        st0 = torch.from_numpy(od_pipe.initial_guess(win))[None]
        ba.BA_window(range(20), INITS, st0, None, *args, 1e-4)
        m1 = ba.snoop_scaled(quantile=SSW.QUANTILE, mode=SSW.MODE, min_rows=SSW.MIN_ROWS)
        last1 = dict(ba.snoop_scaled.last)
        assert tuple(m1.shape) == (1, win.ii.size) and m1.dtype == torch.bool and m1.any()
        ba.restore_rejected()
        m2 = ba.snoop(crit=SSW.QUANTILE, mode=SSW.MODE, min_rows=SSW.MIN_ROWS)
        assert torch.equal(m1, m2) and last1["crit"] == ba.snoop.last["crit"] and last1["counts"] == ba.snoop.last["counts"]
        assert last1["crit"] == SSW.QUANTILE * last1["s0"] and isinstance(last1["flags"], int)
    finally:
        ba.configure(lanes="auto", fusion="auto", solver="auto", mode="auto")
        ba.release()


# ------------------------------------------------------------------------------------------------ error returns
def test_error_returns():
    from test_gpu_parity import _EmulatedRanks
    from vinsat_amd import _lib, od_pipe
    win = _win("C1")
    eng = _engine(win)
    with pytest.raises(_lib.VbaError, match="error 4"):         # before every window has states
        eng.snoop_scaled(12, 3.0)
    eng.set_states(od_pipe.initial_guess(win), 1e-4)
    for q in (0.0, -1.0, np.nan):
        with pytest.raises(_lib.VbaError, match="error 1"):
            eng.snoop_scaled(12, q)
    for kw in (dict(mode=2), dict(mode=-1), dict(min_rows=-1)):
        with pytest.raises(_lib.VbaError, match="error 1"):
            eng.snoop_scaled(12, 3.0, **kw)
    with pytest.raises(_lib.VbaError):
        eng.last_snoop_ms()
    assert not eng.rejected()[0].any()                          # (nothing ran: nothing allocated, nothing rejected)
    eng.close()
    n, m = win.states_gt.shape[0], win.ii.size
    em = _EmulatedRanks(n, m, 2, win.landmarks_xyz, win.landmarks_uv, win.confidences, win.ii, win.intrinsics, win.cumrot_last, win.time_idx)
    em.set_states(od_pipe.initial_guess(win), 1e-4)
    em.call(12, False)
    with pytest.raises(_lib.VbaError, match="error 4"):
        em.engs[0].eng.snoop_scaled(12, 3.0)
    em.close()
