"""vba_outlier_power: minimal detectable biases, external reliabilities, deletion influences, the per-pose summary and the fit
record of every window against the NumPy / SciPy restatement (tests/power_oracle.py) at the GPU's resident states; its chain to
vba_reliability on the same handle; the smallest shapes that can break the row-to-lane mapping; NULL outputs; the scaling
identities that catch a wrong power of the weight; and the promise that the query changes nothing the following calls compute.

Bars.  Against the oracle: 1e-8, max |difference| over the window's largest finite value, per quantity -- the bar of the Sigma
blocks and of vba_reliability.  The dense references differ among themselves (LU against Cholesky,
tests/test_outlier_power_host.py) by at most 5.2e-10 (ext_att, C1), so the bar holds more than three times the spread.  Counts
are compared exactly.  Two solver paths of the covariance step on the same batch: 1e-10, as the covariance paths agree."""
import ctypes

import numpy as np
import pytest

import power_oracle as PO
from query_windows import INITS, SMALL_LAMDA, _ba_args, _batch_engine, _engine, _scheduled, _small_windows, _win

pytestmark = pytest.mark.gpu

ZERO_PIVOT, NONFINITE, INDEFINITE = 4, 2, 8
BAR = 1e-8
ROWS = ("mdb", "ext_pos", "ext_att", "del_pos")
CRIT = 2.0


def _errors(got, ref, m, n):
    """{quantity: error}: rows and the columns of pose_fit over the window's largest finite value, the entries of fit relative;
    the three counts (rows over crit per pose and per window, m_eff) exactly."""
    mdb, ep, ea, dp, pf, fit = got
    e = {k: PO.rel_err_finite(a[:m], ref[k]) for k, a in zip(ROWS, (mdb, ep, ea, dp))}
    for c, name in enumerate(("pose omega", "pose leverage", "pose ext_pos")):
        e[name] = PO.rel_err_finite(pf[:n, c], ref["pose_fit"][:, c])
    assert np.array_equal(pf[:n, 3], ref["pose_fit"][:, 3]) and fit[6] == ref["fit"][6] and fit[1] == ref["fit"][1]
    for c, name in ((0, "Omega"), (2, "t"), (3, "rho"), (4, "s0sq"), (5, "wtest max"), (7, "ext_pos max")):
        if np.isnan(ref["fit"][c]):
            assert np.isnan(fit[c]), name
        else:
            e[name] = abs(fit[c] - ref["fit"][c]) / max(abs(ref["fit"][c]), 1e-300)
    return e


def _check(got, ref, m, n, what, bar=BAR):
    e = _errors(got, ref, m, n)
    print(f"{what}: " + ", ".join(f"{k} {v:.1e}" for k, v in e.items()) + f" (bar {bar:g})")
    assert all(v < bar for v in e.values()), (what, e)


def _assert_no_degenerate_row(ref, dbg):
    live = dbg["w"] > 0
    assert live.all() and (ref["detR"] > 0).all() and (ref["mu_min"] > 0).all()
    assert all(np.isfinite(ref[k]).all() for k in ROWS)


def _query(eng, it, w=0, **kw):
    *out, flags = eng.outlier_power(it, **kw)
    return [a[w] for a in out], flags


@pytest.mark.parametrize("cfg", ["C1", "C2"])
def test_rows_after_the_schedule_against_the_oracle(cfg):
    """Every row array, pose_fit and fit, undamped and damped; the oracle finds no degenerate row on these inputs (asserted)."""
    win = _win(cfg)
    eng = _engine(win)
    st, lam = _scheduled(win, eng)
    n, m = st.shape[0], win.ii.size
    for damped in (False, True):
        ref, dbg = PO.at_states(win, st, lam, damped=damped, crit=CRIT)
        _assert_no_degenerate_row(ref, dbg)
        got, flags = _query(eng, 19, damped=damped, crit=CRIT)
        assert flags[0] & (ZERO_PIVOT | NONFINITE | INDEFINITE) == 0
        _check(got, ref, m, n, f"{cfg} damped={damped}")
        assert got[5][3] > 0 and got[5][6] > 0          # rho; some rows lie over crit = 2, so the counts are not trivially equal
    assert eng.last_outlier_power_ms() > 0.0
    eng.close()


def test_gap_window_and_BA_reg_window_against_the_oracle():
    from conftest import load_golden
    from vinsat_amd import od_pipe, synth
    # the two-pass window (gaps of 935 and 510 s) at the states the reference reached before call 25 (tests/golden/gap.npz)
    g = load_golden("gap")
    win = od_pipe.prepare_window(*synth.make_two_pass_sequence())
    n, m = win.states_gt.shape[0], win.ii.size
    eng = _engine(win)
    eng.set_states(g["states_out_24"][0], float(g["lamda_in"][25]))
    eng.run_schedule([10, 11, 12], [False] * 3)
    st, lam, _, _, _ = eng.get_states()
    ref, dbg = PO.at_states(win, st, lam, it=12, crit=CRIT)
    _assert_no_degenerate_row(ref, dbg)
    got, _ = _query(eng, 12, crit=CRIT)
    _check(got, ref, m, n, "gap window")
    eng.close()
    # BA_reg (the reg_c1 window of the covariance and reliability tests): the prior goes through the oracle's prior= argument
    win = _win("C1")
    n, m = win.states_gt.shape[0], win.ii.size
    rng = np.random.default_rng(6)
    sp = win.states_gt.copy()
    sp[:, :3] += rng.normal(0, 0.5, (n, 3))
    Hs = np.stack([np.eye(6) * s for s in rng.uniform(0.5, 3.0, n)])
    eng = _engine(win)
    eng.upload_prior(sp, Hs)
    eng.set_prior(True)
    st = win.states_gt.copy()
    st[:, :3] += rng.normal(0, 2.0, (n, 3))
    out, lam, _, _, _ = eng.iterate(12, False, 1e-4, st)
    ref, dbg = PO.at_states(win, out, lam, it=12, crit=CRIT, prior=(sp, Hs))
    _assert_no_degenerate_row(ref, dbg)
    got, _ = _query(eng, 12, crit=CRIT)
    _check(got, ref, m, n, "BA_reg window")
    eng.close()


def test_consistent_with_the_reliability_query_of_the_same_handle():
    """pose_fit[..., 1] = pose_stats[..., 0] bit for bit; fit[5] = the maximum of the returned wtest; the counts over crit are
    those of the returned wtest array, per pose and per window; m_eff is the sum of pose_stats[..., 2]."""
    win = _win("C2")
    eng = _engine(win)
    _scheduled(win, eng)
    n, m = win.states_gt.shape[0], win.ii.size
    for damped in (False, True):
        lev, wt, ps, _ = eng.reliability(19, damped=damped, pose_stats=True)
        crit = float(np.median(wt[0, :m]))
        (mdb, ep, ea, dp, pf, fit), _ = _query(eng, 19, damped=damped, crit=crit)
        assert np.array_equal(pf[:n, 1], ps[0, :n, 0])
        assert fit[5] == wt[0, :m].max() == ps[0, :n, 1].max()
        over = wt[0, :m] > crit
        assert 0 < over.sum() < m
        assert np.array_equal(pf[:n, 3], np.bincount(win.ii[over], minlength=n).astype(np.float64))
        assert fit[6] == over.sum() and fit[1] == ps[0, :n, 2].sum() == m
        assert fit[7] == ep[:m].max() == pf[:n, 2].max()
        assert fit[3] == 2.0 * fit[1] - fit[2] and fit[4] == fit[0] / fit[3]
    # crit = None counts nothing
    (_, _, _, _, pf, fit), _ = _query(eng, 19)
    assert (pf[:n, 3] == 0).all() and fit[6] == 0
    eng.close()


# ------------------------------------------------------------------------------------------------ smallest shapes
def test_smallest_shapes_alone_in_a_batch_and_on_both_solver_paths():
    """A 2-pose window with 3 rows on pose 0 and none on pose 1; 17 poses (two blocks of the grid) with 1, 16, 17 and 33 rows on
    poses 0..3; a window with every confidence zero.  Against the oracle with the damping on (undamped, the three rows of the
    first window have no redundancy at all: R_k is singular to rounding, and there is nothing to compare); the batch against each
    window alone bit for bit, damped and undamped; undamped the third window is flagged (and the first), every row of it NaN, s0sq NaN; a chunked
    and the sequential solver setting within 1e-10."""
    wins = _small_windows()
    assert [w.n for w in wins] == [2, 17, 17] and wins[0].m == 3
    assert list(np.bincount(wins[1].ii, minlength=17)[:4]) == [1, 16, 17, 33]
    big = _batch_engine(wins, chunk=0)
    res = {d: big.outlier_power(12, damped=d, crit=CRIT) for d in (True, False)}
    for k, w in enumerate(wins[:2]):
        ref, dbg = PO.at_states(w, w.states0, SMALL_LAMDA, it=12, damped=True, crit=CRIT)
        assert (ref["detR"] > 0).all() and (ref["mu_min"] > 0.01).all()
        _check([a[k] for a in res[True][:6]], ref, w.m, w.n, f"small window {k} ({w.n} poses, {w.m} rows)")
    # the window without weights: flagged undamped, NaN rows, Omega = m_eff = t = 0, s0sq NaN
    mdb, ep, ea, dp, pf, fit, flags = res[False]
    # (so is the 2-pose window: nothing but the chain factors holds its pose without rows)
    assert flags[2] & ZERO_PIVOT and flags[0] & ZERO_PIVOT and not flags[1] & (ZERO_PIVOT | NONFINITE)
    assert all(np.isnan(a[0, :wins[0].m]).all() for a in (mdb, ep, ea, dp)) and np.isnan(fit[0, 4]) and fit[0, 1] == 3.0
    assert all(np.isnan(a[2, :wins[2].m]).all() for a in (mdb, ep, ea, dp))
    assert fit[2, 0] == 0.0 and fit[2, 1] == 0.0 and np.isnan(fit[2, 4]) and fit[2, 5] == 0.0 and fit[2, 7] == 0.0
    # ... and with the damping on it has a Sigma: rows of weight zero give inf, 0, 0, 0
    mdb, ep, ea, dp, pf, fit, flags = res[True]
    assert not flags[2] & (ZERO_PIVOT | NONFINITE)
    assert np.isposinf(mdb[2, :wins[2].m]).all() and all((a[2, :wins[2].m] == 0.0).all() for a in (ep, ea, dp))
    assert np.isnan(fit[2, 4])
    # each window alone: the same bits
    for k, w in enumerate(wins):
        one = _batch_engine([w], chunk=0, sizes=(big.n_max, big.m_max), mode=big.mode()[0])
        for d in (True, False):
            alone = one.outlier_power(12, damped=d, crit=CRIT)
            for a, b, cnt in zip(alone, res[d], (w.m,) * 4 + (w.n, 8, 1)):
                assert np.array_equal(a[0][:cnt] if a.ndim > 1 else a[:1], b[k][:cnt] if b.ndim > 1 else b[k:k + 1], equal_nan=True), (k, d)
        one.close()
    big.close()
    # the partitioned covariance path on the same batch
    other = _batch_engine(wins, chunk=4)
    assert other.mode()[1] == 4
    got = other.outlier_power(12, damped=True, crit=CRIT)
    for k, w in enumerate(wins[:2]):
        for name, a, b, cnt in zip(ROWS + ("pose_fit", "fit"), got, res[True], (w.m,) * 4 + (w.n, 8)):
            x, y = a[k][:cnt], b[k][:cnt]
            err = np.abs(x - y).max() / np.abs(y).max()
            assert err < 1e-10, (k, name, err)
    other.close()


# ------------------------------------------------------------------------------------------------ the query changes nothing
def test_query_changes_nothing_in_a_chained_schedule():
    from vinsat_amd import od_pipe
    win = _win("C1")
    a = _engine(win)
    sa, la = _scheduled(win, a)
    fa = a.get_states()[4]
    b = _engine(win)
    b.set_states(od_pipe.initial_guess(win), 1e-4)
    b.run_schedule(list(range(10)), INITS[:10])
    r0 = b.reliability(9, damped=True, pose_stats=True)
    q0 = b.outlier_power(9, damped=True, crit=CRIT)
    r1 = b.reliability(9, damped=True, pose_stats=True)
    q1 = b.outlier_power(9, damped=True, crit=CRIT)
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(r0, r1))       # the calls around the query: same bits
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(q0, q1))       # equal settings give equal bits
    b.run_schedule(list(range(10, 20)), INITS[10:])
    sb, lb, _, _, fb = b.get_states()
    assert np.array_equal(sa, sb) and la == lb and fa == fb
    a.close()
    b.close()


def test_pipelined_BA_loop_and_BA_window_keep_their_bits():
    import torch
    from vinsat_amd import ba, od_pipe
    win = _win("C1")
    n, m = win.states_gt.shape[0], win.ii.size
    st0 = torch.from_numpy(od_pipe.initial_guess(win))[None]
    common = _ba_args(win)

    def loop(query_at):
        st, lam = st0.clone(), 1e-4
        for it in range(20):
            st, _, lam, _ = ba.BA(it, st, None, *common, 1e-3, 1e-3, lam, None, initialize=it < 10)
            if it == query_at:
                mdb, ep, ea, dp, fit = ba.outlier_power(damped=True, crit=CRIT)
                assert tuple(mdb.shape) == tuple(ep.shape) == tuple(ea.shape) == tuple(dp.shape) == (1, m)
                assert tuple(ba.outlier_power.last["pose_fit"].shape) == (1, n, 4)
                assert fit.dof == 2 * fit.m_eff - fit.leverage_sum and fit.s0 == np.sqrt(fit.s0sq) and fit.dof > 0
        return st.clone(), lam

    ref = loop(-1)
    got = loop(9)
    assert torch.equal(ref[0], got[0]) and ref[1] == got[1]
    ba.release()
    # BA_window (graph replay of the chained schedule): 10 calls + query + 10 calls against 20
    full = ba.BA_window(range(20), INITS, st0, None, *common, 1e-4)
    ba.release()
    half = ba.BA_window(range(10), INITS[:10], st0, None, *common, 1e-4)
    mdb, ep, ea, dp, fit = ba.outlier_power()
    cov = ba.covariance()
    pos, vel, att = ba.scaled_sigmas(cov, fit)
    p0, v0, a0 = ba.pose_sigmas(cov)
    assert torch.equal(pos, p0 * fit.s0) and torch.equal(vel, v0 * fit.s0) and torch.equal(att, a0 * fit.s0)
    rest = ba.BA_window(range(10, 20), INITS[10:], half[0], None, *common, half[2])
    assert torch.equal(full[0], rest[0]) and full[2] == rest[2]
    ba.release()


def test_ragged_batch_through_ba_returns_lists_and_one_record_per_window():
    import torch
    from vinsat_amd import ba, od_pipe
    wins = [_win("C1", seed=s) for s in range(3)]
    sts = [torch.from_numpy(od_pipe.initial_guess(w))[None] for w in wins]
    cols = list(zip(*[_ba_args(w) for w in wins]))
    ba.BA_window(range(12), INITS[:12], sts, None, *[list(x) for x in cols], [1e-4] * 3)
    mdb, ep, ea, dp, fit = ba.outlier_power(crit=CRIT)
    assert isinstance(mdb, list) and len(mdb) == len(fit) == 3
    assert all(tuple(a.shape) == (1, w.ii.size) for a, w in zip(dp, wins))
    assert all(f.m_eff == w.ii.size and f.s0 > 0 for f, w in zip(fit, wins))
    sig = ba.scaled_sigmas(ba.covariance(), fit)
    assert len(sig) == 3 and tuple(sig[1][0].shape) == (1, wins[1].states_gt.shape[0], 3)
    ba.release()


# ------------------------------------------------------------------------------------------------ NULL outputs, bad arguments
def test_null_outputs_in_every_combination_and_bad_arguments():
    from vinsat_amd import _lib, od_pipe
    from vinsat_amd.engine import BAEngine
    wins = [_win("C1", seed=0), _win("C1", seed=1)]
    ns, ms = [w.states_gt.shape[0] for w in wins], [w.ii.size for w in wins]
    N, M = max(ns) + 3, max(ms) + 5
    eng = BAEngine(N, M, windows=2)
    for k, w in enumerate(wins):
        eng.upload_observations(w.landmarks_xyz, w.landmarks_uv, w.confidences, w.ii, ns[k], window=k)
        eng.upload_window(w.intrinsics, w.cumrot_last, w.time_idx, window=k)
        eng.set_states(od_pipe.initial_guess(w), 1e-4, window=k)
    eng.run_schedule(list(range(12)), INITS[:12])
    PD, PU = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint)

    def query(want, ncp=PO.NCP, crit=CRIT):
        outs = [np.full((2, M), -7.0) for _ in range(4)] + [np.full((2, N, 4), -7.0), np.full((2, 8), -7.0)]
        fl = np.full(2, 0xFFFFFFFF, dtype=np.uint32)
        args = [a.ctypes.data_as(PD) if on else None for a, on in zip(outs, want[:6])]
        args.append(fl.ctypes.data_as(PU) if want[6] else None)
        rc = eng.lib.vba_outlier_power(eng.h, 11, 1, ncp, crit, *args)
        return rc, outs + [fl]

    rc, full = query([1] * 7)
    assert rc == 0
    for k in range(2):
        assert all((a[k, ms[k]:] == -7.0).all() and np.isfinite(a[k, :ms[k]]).all() for a in full[:4])
        assert (full[4][k, ns[k]:] == -7.0).all() and np.isfinite(full[4][k, :ns[k]]).all() and np.isfinite(full[5][k]).all()
    assert (full[6] != 0xFFFFFFFF).all()
    masks = [1 << b for b in range(7)] + [0, 0b0101010, 0b1010101]        # each output alone, none, and two mixed sets
    for mask in masks:
        want = [(mask >> b) & 1 for b in range(7)]
        rc, got = query(want)
        assert rc == 0, mask
        for b in range(6):
            assert np.array_equal(got[b], full[b]) if want[b] else (got[b] == -7.0).all(), mask
        assert np.array_equal(got[6], full[6]) if want[6] else (got[6] == 0xFFFFFFFF).all()
    for ncp, crit in ((0.0, CRIT), (-1.0, CRIT), (float("nan"), CRIT), (PO.NCP, 0.0), (PO.NCP, -2.0), (PO.NCP, float("nan"))):
        rc, got = query([1] * 7, ncp=ncp, crit=crit)
        assert rc == 1 and all((a == -7.0).all() for a in got[:6])          # VBA_EINVAL, nothing written
    with pytest.raises(_lib.VbaError, match="error 1"):
        eng.outlier_power(11, ncp=0.0)
    eng.close()


def test_estate_before_states():
    from vinsat_amd import _lib
    win = _win("C1")
    eng = _engine(win)
    with pytest.raises(_lib.VbaError, match="error 4"):
        eng.outlier_power(12)
    eng.close()


# ------------------------------------------------------------------------------------------------ scaling identities
def test_scaling_in_ncp_and_in_the_confidences():
    """Doubling ncp multiplies mdb and ext_* by sqrt(2) to 1 ulp and leaves del_pos and the summaries' bits.  Every confidence times
    0.25: the GPU follows the oracle at the scaled confidences within the bar (the dynamics factors do not scale, so no exact
    factor is asserted -- but the oracle itself shows del_pos and the leverages unchanged within it, Omega and s0sq scaled)."""
    from vinsat_amd import od_pipe
    win = _win("C1")
    n, m = win.states_gt.shape[0], win.ii.size
    eng = _engine(win)
    st, lam = _scheduled(win, eng)
    (mdb, ep, ea, dp, pf, fit), _ = _query(eng, 19)
    (mdb2, ep2, ea2, dp2, pf2, fit2), _ = _query(eng, 19, ncp=2 * PO.NCP)
    # The radicand doubles exactly, so a = sqrt(y) (1 + e1) and b = sqrt(2 y) (1 + e2) with |e| <= 2^-53 each (fp64 square roots
    # are correctly rounded): |b - sqrt(2) a| <= 2^-52 sqrt(2 y), one ulp in the relative sense (an ulp of b lies between 2^-53 b
    # and 2^-52 b).  The product sqrt(2) a is formed in extended precision: in fp64 it would carry an ulp of its own.
    root2 = np.sqrt(np.longdouble(2.0))
    ulp = np.longdouble(2.0) ** -52
    for a, b in ((mdb, mdb2), (ep, ep2), (ea, ea2)):
        want = root2 * a[:m].astype(np.longdouble)
        assert (np.abs(b[:m].astype(np.longdouble) - want) <= ulp * want).all()
    assert np.array_equal(dp[:m], dp2[:m]) and np.array_equal(pf[:n, :2], pf2[:n, :2]) and np.array_equal(fit[:7], fit2[:7])
    assert abs(np.longdouble(fit2[7]) - root2 * np.longdouble(fit[7])) <= ulp * fit2[7]
    # confidences times 0.25, same states
    conf = 0.25 * win.confidences
    eng.upload_observations(win.landmarks_xyz, win.landmarks_uv, conf, win.ii, n)
    eng.set_states(st, lam)
    got, _ = _query(eng, 19, crit=CRIT)
    ref, _ = PO.at_states(win, st, lam, crit=CRIT, conf=conf)
    _check(got, ref, m, n, "C1, confidences x 0.25")
    base, _ = PO.at_states(win, st, lam, crit=CRIT)
    e_dp, e_lev = PO.rel_err_finite(got[3][:m], base["del_pos"]), PO.rel_err_finite(got[4][:n, 1], base["pose_fit"][:, 1])
    print(f"confidences x 0.25 against the unscaled oracle: del_pos {e_dp:.1e}, pose leverage sums {e_lev:.1e}; "
          f"Omega ratio {got[5][0] / base['fit'][0]:.6f}, s0sq ratio {got[5][4] / base['fit'][4]:.6f}")
    assert abs(got[5][0] / base["fit"][0] - ref["fit"][0] / base["fit"][0]) < BAR
    assert abs(got[5][4] / base["fit"][4] - ref["fit"][4] / base["fit"][4]) < BAR
    eng.close()
