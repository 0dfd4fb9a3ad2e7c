"""vba_reliability: per-row leverages and standardised residuals (w-tests) and the per-pose summary against the NumPy restatement
(tests/rel_oracle.py) at the GPU's resident states, the exact chain to the covariance query and VBA_DBG_H, a planted blunder, and
the promise that the query changes nothing the following calls compute.

Bars.  Rows against the oracle: 1e-8, max|d| over the rows over the window's largest value -- the bar the Sigma blocks carry
(tests/test_gpu_covariance.py); leverages are linear in those blocks.  The dense references differ among themselves (LU against
Cholesky, tests/test_reliability_host.py) by 8.4e-11 (leverage) and 4.5e-12 (wtest) at C1, 4.8e-12 / 5.0e-14 at C2: the bar holds
more than three times that.  Exact chain (same Sigma, same weights, sums in another order): 1e-10."""
import ctypes

import numpy as np
import pytest

import rel_oracle as R
from query_windows import INITS, _ba_args, _engine, _scheduled, _win

pytestmark = pytest.mark.gpu

ZERO_PIVOT, NONFINITE, INDEFINITE = 4, 2, 8
BAR = 1e-8


def _assert_no_degenerate_row(ref, dbg):
    ev = np.linalg.eigvalsh(ref["P"])
    assert dbg["w"].min() > 0.0 and ev.min() > 0.0 and ev.max() < 1.0
    assert np.isfinite(ref["wtest"]).all() and np.isfinite(ref["leverage"]).all()


def _check_rows(got, ref, m, n, what):
    lev, wt, ps = got
    e_l, e_t = R.row_rel_err(lev[:m], ref["leverage"]), R.row_rel_err(wt[:m], ref["wtest"])
    e_s = R.row_rel_err(ps[:n, 0], ref["pose_stats"][:, 0])
    print(f"{what}: leverage {e_l:.2e}, wtest {e_t:.2e}, pose sums {e_s:.2e} (bar {BAR:g})")
    assert e_l < BAR and e_t < BAR and e_s < BAR, (what, e_l, e_t, e_s)
    assert np.array_equal(ps[:n, 2], ref["pose_stats"][:, 2])


@pytest.mark.parametrize("cfg", ["C1", "C2", "C3"])
def test_rows_after_the_schedule_against_the_oracle(cfg):
    """Every row, undamped and damped; the reference has no degenerate row on these inputs (asserted through the oracle)."""
    win = _win(cfg)
    eng = _engine(win)
    st, lam = _scheduled(win, eng)
    n, m = st.shape[0], win.ii.size
    for damped in (False, True):
        ref, dbg = R.at_states(win, st, lam, damped=damped)
        _assert_no_degenerate_row(ref, dbg)
        lev, wt, ps, flags = eng.reliability(19, damped=damped, pose_stats=True)
        assert flags[0] & (ZERO_PIVOT | NONFINITE | INDEFINITE) == 0
        _check_rows((lev[0], wt[0], ps[0]), ref, m, n, f"{cfg} damped={damped}")
        assert (lev[0, :m] > 0).all() and (lev[0, :m] < 2).all()
    assert eng.last_reliability_ms() > 0.0
    eng.close()


def test_exact_chain_to_the_covariance_query_and_the_next_calls_H():
    """pose_stats[:, 0] = tr(S_i H_i) with S from the covariance query of the same handle and H = VBA_DBG_H of one more call from
    the same states (pipeline off); the counts are those of ii; the maxima are those of the returned wtest, bit for bit."""
    win = _win("C2")
    eng = _engine(win)
    eng.set_pipeline(False)
    st, lam = _scheduled(win, eng)
    n, m = st.shape[0], win.ii.size
    lev, wt, ps, _ = eng.reliability(19, pose_stats=True)
    diag, _ = eng.covariance(19)
    eng.step(19, False)
    H = eng.debug("H")
    tr = np.einsum("iab,iba->i", diag[0, :n, :6, :6], H)
    err = np.abs(ps[0, :n, 0] - tr).max() / np.abs(tr).max()
    print(f"exact chain: max |sum leverage - tr(S H)| / max = {err:.2e}")
    assert err < 1e-10
    assert np.array_equal(ps[0, :n, 2], np.bincount(win.ii, minlength=n).astype(np.float64))
    mx = np.array([wt[0, :m][win.ii == i].max() for i in range(n)])
    assert np.array_equal(ps[0, :n, 1], mx)
    # the row sums too, in the kernel's order or any other: rounding only
    sums = np.bincount(win.ii, weights=lev[0, :m], minlength=n)
    assert np.abs(ps[0, :n, 0] - sums).max() <= 1e-13 * np.abs(sums).max()
    eng.close()


def test_a_blunder_of_200_px_has_the_largest_wtest_in_input_order():
    """Rows shuffled (not pose sorted: the index that comes back is one of the input order), one row's uv moved by 200 px before the
    upload."""
    win = _win("C2")
    rng = np.random.default_rng(11)
    m, n = win.ii.size, win.states_gt.shape[0]
    order = rng.permutation(m)
    xyz, uv, conf, ii = win.landmarks_xyz[order], win.landmarks_uv[order].copy(), win.confidences[order], win.ii[order]
    assert (np.diff(ii) < 0).any()
    bad = int(rng.integers(m))

    def run(uv_):
        from vinsat_amd import od_pipe
        from vinsat_amd.engine import BAEngine
        eng = BAEngine(n, m)
        eng.upload_observations(xyz, uv_, conf, ii, n)
        eng.upload_window(win.intrinsics, win.cumrot_last, win.time_idx)
        eng.set_states(od_pipe.initial_guess(win), 1e-4)
        eng.run_schedule(list(range(20)), INITS)
        _, wt, fl = eng.reliability(19)
        eng.close()
        assert fl[0] & (ZERO_PIVOT | NONFINITE) == 0 and np.isfinite(wt[0, :m]).all()
        return wt[0, :m]

    clean = run(uv)
    uv_bad = uv.copy()
    uv_bad[bad] += np.array([200.0, 0.0])
    wt = run(uv_bad)
    rest = np.delete(wt, bad)
    print(f"blunder row {bad}: wtest {wt[bad]:.3g}; rest max {rest.max():.3g}, 99.9th percentile {np.percentile(rest, 99.9):.3g}; "
          f"clean window max {clean.max():.3g}")
    assert int(np.argmax(wt)) == bad
    assert wt[bad] > np.percentile(rest, 99.9)
    assert clean.max() < wt[bad]


def test_query_changes_nothing_in_a_chained_schedule_and_keeps_the_covariance_bits():
    from vinsat_amd import od_pipe
    win = _win("C2")
    a = _engine(win)
    sa, la = _scheduled(win, a)
    b = _engine(win)
    b.set_states(od_pipe.initial_guess(win), 1e-4)
    b.run_schedule(list(range(10)), INITS[:10])
    c0 = b.covariance(9, damped=True, super_diagonal=True)
    b.reliability(9, damped=True, pose_stats=True)
    c1 = b.covariance(9, damped=True, super_diagonal=True)
    assert all(np.array_equal(x, y) for x, y in zip(c0, c1))
    b.run_schedule(list(range(10, 20)), INITS[10:])
    sb, lb, _, _, _ = b.get_states()
    assert np.array_equal(sa, sb) and la == lb
    a.close()
    b.close()


def test_pipelined_BA_loop_keeps_its_bits():
    import torch
    from vinsat_amd import ba, od_pipe
    win = _win("C1")
    st0 = torch.from_numpy(od_pipe.initial_guess(win))[None]
    imu = np.zeros((1, st0.shape[1], 2, 10))
    imu[0, :, -1, 6:10] = win.cumrot_last
    common = (imu, win.landmarks_uv[None], win.landmarks_xyz[None], win.ii, win.time_idx, win.intrinsics[None], win.confidences)

    def loop(query_at):
        st, lam = st0.clone(), 1e-4
        for it in range(20):
            st, _, lam, _ = ba.BA(it, st, None, *common, 1e-3, 1e-3, lam, None, initialize=it < 10)
            if it == query_at:
                lev, wt = ba.reliability(damped=True)
                assert tuple(lev.shape) == tuple(wt.shape) == (1, win.ii.size)
        return st.clone(), lam

    ref = loop(-1)
    got = loop(9)
    assert torch.equal(ref[0], got[0]) and ref[1] == got[1]
    ba.release()


def test_window_alone_and_as_window_3_of_a_ragged_batch_at_pinned_settings():
    import torch
    from vinsat_amd import ba, od_pipe, synth
    cfgs = ["C1", "C2", "C1", "C2", "C1"]
    wins = [_win(c, seed=s) for s, c in enumerate(cfgs)]
    sts = [torch.from_numpy(od_pipe.initial_guess(w))[None] for w in wins]
    ba.configure(lanes=8, fusion=12, solver=(8, -1), mode="lat")
    try:
        cols = list(zip(*[_ba_args(w) for w in wins]))
        out = ba.BA_window(range(20), INITS, sts, None, *[list(x) for x in cols], [1e-4] * 5)
        lev, wt = ba.reliability()
        psb = ba.reliability.last["pose_stats"]
        assert isinstance(lev, list) and len(lev) == 5 and len(ba.reliability.last["flags"]) == 5
        for k, w in enumerate(wins):
            assert tuple(lev[k].shape) == tuple(wt[k].shape) == (1, w.ii.size)
            assert tuple(psb[k].shape) == (1, w.states_gt.shape[0], 3)
        ba.release()
        one = ba.BA_window(range(20), INITS, sts[3], None, *_ba_args(wins[3]), 1e-4)
        assert torch.equal(one[0], out[0][3])
        l1, t1 = ba.reliability()
        assert torch.equal(l1, lev[3]) and torch.equal(t1, wt[3])
        assert torch.equal(ba.reliability.last["pose_stats"], psb[3])
    finally:
        ba.configure(lanes="auto", fusion="auto", solver="auto", mode="auto")
        ba.release()


def test_rows_and_poses_beyond_a_windows_counts_are_untouched_and_null_outputs_accepted():
    from vinsat_amd import _lib, od_pipe
    from vinsat_amd.engine import BAEngine
    wins = [_win("C1", seed=0), _win("C2", seed=1), _win("C1", seed=2)]
    ns, ms = [w.states_gt.shape[0] for w in wins], [w.ii.size for w in wins]
    N, M = max(ns) + 3, max(ms) + 5
    eng = BAEngine(N, M, windows=3)
    for k, w in enumerate(wins):
        eng.upload_observations(w.landmarks_xyz, w.landmarks_uv, w.confidences, w.ii, ns[k], window=k)
        eng.upload_window(w.intrinsics, w.cumrot_last, w.time_idx, window=k)
        eng.set_states(od_pipe.initial_guess(w), 1e-4, window=k)
    eng.run_schedule(list(range(12)), INITS[:12])
    PD, PU = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint)

    def query(want):
        lev, wt, ps = np.full((3, M), -7.0), np.full((3, M), -7.0), np.full((3, N, 3), -7.0)
        fl = np.full(3, 0xFFFFFFFF, dtype=np.uint32)
        args = [a.ctypes.data_as(PD) if on else None for a, on in zip((lev, wt, ps), want[:3])]
        args.append(fl.ctypes.data_as(PU) if want[3] else None)
        _lib.check(eng.lib.vba_reliability(eng.h, 11, 1, *args), eng.lib)
        return lev, wt, ps, fl

    full = query((1, 1, 1, 1))
    for k in range(3):
        assert (full[0][k, ms[k]:] == -7.0).all() and (full[1][k, ms[k]:] == -7.0).all() and (full[2][k, ns[k]:] == -7.0).all()
        assert (full[0][k, :ms[k]] > 0).all() and np.isfinite(full[1][k, :ms[k]]).all() and (full[2][k, :ns[k], 2] > 0).all()
    assert (full[3] != 0xFFFFFFFF).all()
    for mask in range(16):
        want = [(mask >> b) & 1 for b in range(4)]
        got = query(want)
        for b in range(3):
            assert np.array_equal(got[b], full[b]) if want[b] else (got[b] == -7.0).all(), mask
        assert np.array_equal(got[3], full[3]) if want[3] else (got[3] == 0xFFFFFFFF).all()
    # each window alone: same bits (no setting of the handle reaches the row pass; the states are handed over)
    S, lams, _, _, _ = eng.get_states_all()
    for k, w in enumerate(wins):
        one = BAEngine(N, M, windows=1, mode=eng.mode()[0])
        one.set_solver(eng.mode()[1])
        one.upload_observations(w.landmarks_xyz, w.landmarks_uv, w.confidences, w.ii, ns[k])
        one.upload_window(w.intrinsics, w.cumrot_last, w.time_idx)
        one.set_states(S[k, :ns[k]], lams[k])
        l1, t1, p1, f1 = one.reliability(11, damped=True, pose_stats=True)
        assert np.array_equal(l1[0, :ms[k]], full[0][k, :ms[k]]) and np.array_equal(t1[0, :ms[k]], full[1][k, :ms[k]])
        assert np.array_equal(p1[0, :ns[k]], full[2][k, :ns[k]]) and f1[0] == full[3][k]
        one.close()
    eng.close()


def test_a_row_of_confidence_zero_returns_zeros():
    win = _win("C1")
    conf = win.confidences.copy()
    conf[7] = 0.0
    eng = _engine(win)
    n = win.states_gt.shape[0]
    eng.upload_observations(win.landmarks_xyz, win.landmarks_uv, conf, win.ii, n)
    _scheduled(win, eng)
    lev, wt, ps, fl = eng.reliability(19, pose_stats=True)
    assert lev[0, 7] == 0.0 and wt[0, 7] == 0.0
    assert ps[0, win.ii[7], 2] == np.count_nonzero(win.ii == win.ii[7]) - 1
    others = np.delete(np.arange(win.ii.size), 7)
    assert (lev[0, others] > 0).all() and np.isfinite(wt[0, others]).all()
    eng.close()


def test_a_window_without_a_covariance_returns_nan_wtest_and_the_flag():
    """The issue names a one-pose undamped window.  The library takes no such window (vba_upload_observations: 2 <= n), which is
    asserted here; the flagged path runs on the singular window that does exist, the one of tests/test_gpu_covariance.py (all
    confidences zero, undamped), on both paths of the covariance step: VBA_FLAG_ZERO_PIVOT, every wtest NaN, leverages of the weight-zero rows 0."""
    from vinsat_amd import _lib, od_pipe
    from vinsat_amd.engine import BAEngine
    win = _win("C1")
    n, m = win.states_gt.shape[0], win.ii.size
    one = BAEngine(n, m)
    sel = win.ii == 0
    with pytest.raises(_lib.VbaError):
        one.upload_observations(win.landmarks_xyz[sel], win.landmarks_uv[sel], win.confidences[sel], win.ii[sel], 1)
    one.close()
    for chunk in (0, -1):
        eng = _engine(win)
        eng.set_solver(chunk)
        eng.upload_observations(win.landmarks_xyz, win.landmarks_uv, np.zeros_like(win.confidences), win.ii, n)
        eng.set_states(od_pipe.initial_guess(win), 1e-4)
        lev, wt, ps, fl = eng.reliability(12, damped=False, pose_stats=True)
        assert fl[0] & ZERO_PIVOT
        assert np.isnan(wt[0, :m]).all() and (lev[0, :m] == 0.0).all()
        assert (ps[0, :n, 1] == 0.0).all() and (ps[0, :n, 2] == 0.0).all()
        eng.close()


def test_estate_before_states_and_on_a_sharded_handle():
    from test_gpu_parity import _EmulatedRanks
    from vinsat_amd import _lib, od_pipe
    win = _win("C1")
    eng = _engine(win)
    with pytest.raises(_lib.VbaError, match="error 4"):
        eng.reliability(12)
    eng.close()
    n, m = win.states_gt.shape[0], win.ii.size
    em = _EmulatedRanks(n, m, 2, win.landmarks_xyz, win.landmarks_uv, win.confidences, win.ii, win.intrinsics, win.cumrot_last, win.time_idx)
    em.set_states(od_pipe.initial_guess(win), 1e-4)
    em.call(12, False)
    with pytest.raises(_lib.VbaError, match="error 4"):
        em.engs[0].eng.reliability(12)
    em.close()


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
    ref, dbg = R.at_states(win, st, lam, it=12)
    _assert_no_degenerate_row(ref, dbg)
    lev, wt, ps, fl = eng.reliability(12, pose_stats=True)
    _check_rows((lev[0], wt[0], ps[0]), ref, m, n, "gap window")
    eng.close()
    # BA_reg: the prior goes through the oracle's prior= argument
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
    ref, dbg = R.at_states(win, out, lam, it=12, prior=(sp, Hs))
    _assert_no_degenerate_row(ref, dbg)
    lev, wt, ps, fl = eng.reliability(12, pose_stats=True)
    _check_rows((lev[0], wt[0], ps[0]), ref, m, n, "BA_reg window")
    eng.close()


def test_ba_reliability_shapes_and_streaming_record(monkeypatch):
    import torch
    from vinsat_amd import ba, od_pipe, synth
    wins = [_win("C1", seed=s) for s in range(3)]
    sts = [torch.from_numpy(od_pipe.initial_guess(w))[None] for w in wins]
    n0, m0 = sts[0].shape[1], wins[0].ii.size
    a0 = _ba_args(wins[0])
    # BA, one window
    ba.BA(11, sts[0], None, *a0, 1e-3, 1e-3, 1e-4, None, initialize=False)
    lev, wt = ba.reliability()
    assert tuple(lev.shape) == tuple(wt.shape) == (1, m0) and lev.dtype == torch.float64
    assert tuple(ba.reliability.last["pose_stats"].shape) == (1, n0, 3) and isinstance(ba.reliability.last["flags"], int)
    # BA_reg
    sp = wins[0].states_gt[None].copy()
    Hs = np.stack([np.eye(6)] * n0)[None]
    ba.BA_reg(11, sts[0], None, sp, None, Hs, None, *a0, 1e-3, 1e-3, 1e-4, None, initialize=False)
    lr, tr = ba.reliability(damped=True)
    assert tuple(lr.shape) == (1, m0) and not torch.equal(lr, lev)      # (the prior is in the system)
    # BA_window, ragged batch
    cols = list(zip(*[_ba_args(w) for w in wins]))
    ba.BA_window(range(12), INITS[:12], sts, None, *[list(x) for x in cols], [1e-4] * 3)
    ll, tl = ba.reliability()
    assert isinstance(ll, list) and len(ll) == len(tl) == 3
    assert all(tuple(l.shape) == (1, w.ii.size) for l, w in zip(ll, wins))
    assert len(ba.reliability.last["flags"]) == 3 and len(ba.reliability.last["pose_stats"]) == 3
    # dense batch
    dense = torch.cat([sts[0]] * 2)
    ba.BA(11, dense, None, np.concatenate([a0[0]] * 2), np.concatenate([a0[1]] * 2), np.concatenate([a0[2]] * 2), a0[3], a0[4],
          np.concatenate([a0[5]] * 2), a0[6], 1e-3, 1e-3, [1e-4, 1e-4], None, initialize=False)
    ld, td = ba.reliability()
    assert tuple(ld.shape) == tuple(td.shape) == (2, m0) and torch.equal(ld[0], ld[1]) and torch.equal(td[0], td[1])
    assert tuple(ba.reliability.last["pose_stats"].shape) == (2, n0, 3)
    ba.release()
    # streaming driver: one entry per batch with one value per row of that batch; the results bit for bit as without the list
    det, orb = synth.make_two_pass_sequence()
    e0, f0, t0 = od_pipe.streaming_version(det, orb)
    ba.release()
    rows = []
    real = ba.BA_window

    def counting(iters, inits, states, vel, imu, uv, *rest):
        rows.append(int(np.asarray(uv).reshape(-1, 2).shape[0]))
        return real(iters, inits, states, vel, imu, uv, *rest)

    monkeypatch.setattr(ba, "BA_window", counting)
    rel = []
    e1, f1, t1 = od_pipe.streaming_version(det, orb, reliability=rel)
    monkeypatch.setattr(ba, "BA_window", real)
    assert torch.equal(e0, e1) and f0 == f1 and all(np.array_equal(a, b) for a, b in zip(t0, t1))
    assert len(rel) == len(rows) >= 1
    for r, m in zip(rel, rows):
        assert tuple(r["leverage"].shape) == tuple(r["wtest"].shape) == (m,)
    ba.release()
    # batched driver: round and sequence like the covariances
    seqs = [synth.make_two_pass_sequence(), synth.make_sequence("C1")]
    ref = od_pipe.streaming_batched(seqs)
    ba.release()
    rel = []
    got = od_pipe.streaming_batched(seqs, reliability=rel)
    ba.release()
    for (e0, f0, t0), (e1, f1, t1) in zip(ref, got):
        assert torch.equal(e0, e1) and f0 == f1 and all(np.array_equal(a, b) for a, b in zip(t0, t1))
    rounds = {}
    for r in rel:
        assert r["leverage"].shape == r["wtest"].shape and r["leverage"].ndim == 1
        rounds.setdefault(r["round"], []).append(r["sequence"])
    assert rounds[0] == [0, 1] and all(sorted(v) == sorted(set(v)) for v in rounds.values())
