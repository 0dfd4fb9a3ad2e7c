"""vba_covariance: per-pose marginal covariances (diagonal and super-diagonal blocks of the inverse of the symmetrised full-phase
system at the resident states) against NumPy inverses of the oracle's system (tests/cov_oracle.py), and the promise that the
query changes nothing the following calls compute.

Bars.  The system is ill-conditioned (condition ~1e11 at C1 after the 20-call schedule, ~6e10 at C2), and the dense NumPy references
disagree among themselves by up to 2.1e-9 per-pose block error (LU inverse vs Cholesky on identity columns, C1 damped; 7.8e-11 at
C2), the block recurrence by 1.0e-9 (tests/test_covariance_host.py).  Blocks against the oracle: 1e-8 per pose (max|dS_ii| / max|S_ii|);
per-component sigmas: 3e-9 relative (the references differ by 1.0e-9 in sigma on C1: the issue's 1e-9 lies inside that spread, the
bar is three times it).
Against the inverse of the library's own bands (same system to rounding): 1e-10."""
import numpy as np
import pytest

import cov_oracle as C
from oracle import ba_oracle as O
from query_windows import INITS, _engine, _scheduled, _win

pytestmark = pytest.mark.gpu

ZERO_PIVOT, INDEFINITE = 4, 8


def _oracle_bands(win, st, lam, it=19, **kw):
    d = {}
    O.ba_iteration(it, st, win.cumrot_last, win.landmarks_uv, win.landmarks_xyz, win.ii, win.time_idx, win.intrinsics,
                   win.confidences, lam, initialize=False, debug=d, **kw)
    return d["bands"]


def _check_against(bands, lam, diag, sup, n, bar=1e-8, sbar=3e-9, dense=True):
    ref = C.marginal_dense(bands, lam) if dense else C.marginal_blocks(bands, lam)
    e_d, e_s, e_sig = C.block_rel_err(diag[:n], ref[0]), C.block_rel_err(sup[:n - 1], ref[1][:n - 1]), C.sigma_rel_err(diag[:n], ref[0])
    assert e_d < bar and e_s < bar and e_sig < sbar, (e_d, e_s, e_sig)
    assert not sup[n - 1].any()


@pytest.mark.parametrize("cfg", ["C1", "C2", "C3"])
def test_marginals_after_the_schedule_against_the_oracle(cfg):
    win = _win(cfg)
    eng = _engine(win)
    st, lam = _scheduled(win, eng)
    n = st.shape[0]
    bands = _oracle_bands(win, st, lam)
    for damped in (False, True):
        diag, sup, flags = eng.covariance(19, damped=damped, super_diagonal=True)
        assert flags[0] & (ZERO_PIVOT | INDEFINITE) == 0
        _check_against(bands, float(np.float32(lam)) if damped else 0.0, diag[0], sup[0], n)
        assert np.array_equal(diag[0, :n], diag[0, :n].transpose(0, 2, 1))     # one triangle, mirrored
    assert eng.last_covariance_ms() > 0.0
    eng.close()


def test_query_is_the_inverse_of_the_next_calls_own_bands():
    """One more call from the same resident states (pipeline off, so its intermediates stay readable): its VBA_DBG_BANDS,
    symmetrised and inverted, equal the sequential walk's query to 1e-10, and the partitioned path (this handle's default) equals the
    walk to 1e-10.  Measured on C2: walk against the LU inverse within the bar; partitioned against it 1.11e-10 per-pose block error,
    where the dense references themselves (LU against Cholesky) differ by 7.8e-11 -- the partitioned path is held to 1e-10 against the
    walk (here and in test_sequential_and_partitioned_paths_agree), not against a reference that is no more accurate than the bar.
    And A - A^T beyond rounding lives in the rot-rot diagonal blocks only (the oracle's own bands differ from their transpose by
    ~1e-16 of the largest entry elsewhere: the cross blocks are formed apart)."""
    win = _win("C2")
    eng = _engine(win)
    eng.set_pipeline(False)
    st, lam = _scheduled(win, eng)
    n = st.shape[0]
    assert eng.mode()[1] > 0
    dp, spp, _ = eng.covariance(19, damped=False, super_diagonal=True)
    eng.set_solver(0)
    diag, sup, flags = eng.covariance(19, damped=False, super_diagonal=True)
    assert C.block_rel_err(dp[0, :n], diag[0, :n]) < 1e-10 and C.block_rel_err(spp[0, :n - 1], sup[0, :n - 1]) < 1e-10
    eng.step(19, False)
    bands = eng.debug("bands")
    _check_against(bands, 0.0, diag[0], sup[0], n, bar=1e-10, sbar=1e-10)
    # A - A^T: rounding outside the rot-rot diagonal blocks (E^T F / F^T E and Hu / Hl are formed apart, as in the oracle)
    scale = np.abs(bands).max()
    for i in range(n):
        d = bands[i, 1] - bands[i, 1].T
        d[3:6, 3:6] = 0.0
        assert np.abs(d).max() <= 1e-13 * scale, i
        if i + 1 < n:
            assert np.abs(bands[i, 2] - bands[i + 1, 0].T).max() <= 1e-13 * scale, i
    eng.close()


def test_query_changes_nothing_in_a_chained_schedule():
    win = _win("C2")
    a = _engine(win)
    sa, la = _scheduled(win, a)
    b = _engine(win)
    from vinsat_amd import od_pipe
    b.set_states(od_pipe.initial_guess(win), 1e-4)
    b.run_schedule(list(range(10)), INITS[:10])
    b.covariance(9, damped=True)
    b.run_schedule(list(range(10, 20)), INITS[10:])
    sb, lb, _, _, _ = b.get_states()
    assert np.array_equal(sa, sb) and la == lb
    a.close()
    b.close()


def test_python_loops_with_pipelining_and_graph_replay_keep_their_bits():
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
                cov = ba.covariance(damped=True)
                assert tuple(cov.shape) == (1, st0.shape[1], 9, 9)
        return st.clone(), lam

    ref = loop(-1)
    got = loop(9)
    assert torch.equal(ref[0], got[0]) and ref[1] == got[1]
    # BA_window (graph replay): 10 + query + 10 against one 20-call window
    w20 = ba.BA_window(range(20), INITS, st0.clone(), None, *common, 1e-4)
    w10 = ba.BA_window(range(10), INITS[:10], st0.clone(), None, *common, 1e-4)
    ba.covariance()
    w10b = ba.BA_window(range(10, 20), INITS[10:], w10[0], None, *common, w10[2])
    assert torch.equal(w20[0], w10b[0]) and w20[2] == w10b[2]
    assert torch.equal(w20[0], ref[0])
    ba.release()


def _gap_window():
    from vinsat_amd import od_pipe, synth
    return od_pipe.prepare_window(*synth.make_two_pass_sequence())


def test_gap_window_against_the_oracle_and_without_side_effects():
    win = _gap_window()
    st = win.states_gt.copy()
    st[:, :3] += 0.5
    n = st.shape[0]

    def run(query):
        eng = _engine(win)
        eng.set_states(st, 1e-3)
        eng.run_schedule([10, 11, 12], [False] * 3)
        res = None
        if query:
            s_mid, l_mid, _, _, _ = eng.get_states()
            res = (s_mid, l_mid) + eng.covariance(12, damped=False, super_diagonal=True)
        eng.run_schedule([13, 14], [False] * 2)
        out = eng.get_states()[:2]
        eng.close()
        return out, res

    ref, _ = run(False)
    got, (s_mid, l_mid, diag, sup, flags) = run(True)
    assert np.array_equal(ref[0], got[0]) and ref[1] == got[1]
    _check_against(_oracle_bands(win, s_mid, l_mid, it=12), 0.0, diag[0], sup[0], n)


def test_hop_integrator_and_prior_against_the_oracle():
    win = _win("C1")
    n = win.states_gt.shape[0]
    # hop integrator
    eng = _engine(win)
    eng.set_integrator(True)
    from vinsat_amd import od_pipe
    eng.set_states(od_pipe.initial_guess(win), 1e-4)
    eng.run_schedule(list(range(20)), INITS)
    st, lam, _, _, _ = eng.get_states()
    diag, sup, _ = eng.covariance(19, damped=True, super_diagonal=True)
    _check_against(_oracle_bands(win, st, lam, hop=True), float(np.float32(lam)), diag[0], sup[0], n)
    eng.close()
    # BA_reg prior (reg_c1)
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
    diag, sup, _ = eng.covariance(12, damped=False, super_diagonal=True)
    _check_against(_oracle_bands(win, out, lam, it=12, prior=(sp, Hs)), 0.0, diag[0], sup[0], n)
    eng.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_ragged_batch_has_the_bits_of_each_window_alone(mode):
    from vinsat_amd import od_pipe
    from vinsat_amd.engine import BAEngine
    wins = [_win("C1", seed=s) for s in range(4)]
    ns = [w.states_gt.shape[0] for w in wins]
    ms = [w.ii.size for w in wins]
    big = BAEngine(max(ns), max(ms), windows=4, mode=mode)
    for k, w in enumerate(wins):
        big.upload_observations(w.landmarks_xyz, w.landmarks_uv, w.confidences, w.ii, ns[k], window=k)
        big.upload_window(w.intrinsics, w.cumrot_last, w.time_idx, window=k)
        big.set_states(od_pipe.initial_guess(w), 1e-4, window=k)
    big.run_schedule(list(range(12)), INITS[:12])
    S, lams, _, _, _ = big.get_states_all()
    dg, sp, fl = big.covariance(11, damped=True, super_diagonal=True)
    for k, w in enumerate(wins):
        one = BAEngine(max(ns), max(ms), windows=1, mode=mode)
        one.upload_observations(w.landmarks_xyz, w.landmarks_uv, w.confidences, w.ii, ns[k])
        one.upload_window(w.intrinsics, w.cumrot_last, w.time_idx)
        one.set_states(S[k, :ns[k]], lams[k])
        d1, s1, f1 = one.covariance(11, damped=True, super_diagonal=True)
        assert np.array_equal(d1[0, :ns[k]], dg[k, :ns[k]]) and np.array_equal(s1[0, :ns[k]], sp[k, :ns[k]]) and f1[0] == fl[k]
        one.close()
    big.close()


@pytest.mark.parametrize("chunk", [0, -1])
def test_singular_window_reports_a_zero_pivot_and_nan_blocks(chunk):
    """All confidences zero: no observation information, positions and attitudes are free up to the chain factors -- the undamped
    system is singular.  Both paths (chunk 0: sequential walk; -1: the default, a partitioned solve of this 10-pose window)."""
    from vinsat_amd import od_pipe
    win = _win("C1")
    eng = _engine(win)
    eng.set_solver(chunk)
    assert (eng.mode()[1] == 0) == (chunk == 0)
    eng.upload_observations(win.landmarks_xyz, win.landmarks_uv, np.zeros_like(win.confidences), win.ii, win.states_gt.shape[0])
    eng.set_states(od_pipe.initial_guess(win), 1e-4)
    diag, sup, flags = eng.covariance(12, damped=False, super_diagonal=True)
    n = win.states_gt.shape[0]
    assert flags[0] & ZERO_PIVOT
    assert np.isnan(diag[0, :n]).all() and np.isnan(sup[0, :n - 1]).all() and not sup[0, n - 1].any()
    eng.close()


def test_C5_against_the_block_recurrence():
    win = _win("C5")
    eng = _engine(win)
    st, lam = _scheduled(win, eng, calls=12)
    n = st.shape[0]
    diag, sup, flags = eng.covariance(11, damped=True, super_diagonal=True)
    _check_against(_oracle_bands(win, st, lam, it=11), float(np.float32(lam)), diag[0], sup[0], n, dense=False)
    eng.close()


def test_ba_covariance_forms_and_streaming_record():
    import torch
    from vinsat_amd import ba, od_pipe, synth
    wins = [_win("C1", seed=s) for s in range(3)]

    def args(w):
        imu = np.zeros((1, w.states_gt.shape[0], 2, 10))
        imu[0, :, -1, 6:10] = w.cumrot_last
        return imu, w.landmarks_uv[None], w.landmarks_xyz[None], w.ii, w.time_idx, w.intrinsics[None], w.confidences

    sts = [torch.from_numpy(od_pipe.initial_guess(w))[None] for w in wins]
    ba.BA(0, sts[0], None, *args(wins[0]), 1e-3, 1e-3, 1e-4, None, initialize=True)
    c = ba.covariance()
    assert tuple(c.shape) == (1, sts[0].shape[1], 9, 9) and c.dtype == torch.float64
    d, s = ba.covariance(damped=True, super_diagonal=True)
    assert d.shape == s.shape
    pos, vel, att = ba.pose_sigmas(c)
    assert tuple(pos.shape) == (1, sts[0].shape[1], 3)
    # ragged batch
    cols = list(zip(*[args(w) for w in wins]))
    ba.BA_window(range(3), [True] * 3, sts, None, *[list(x) for x in cols], [1e-4] * 3)
    cl = ba.covariance()
    assert isinstance(cl, list) and len(cl) == 3 and tuple(cl[1].shape) == (1, sts[1].shape[1], 9, 9)
    assert len(ba.covariance.last["flags"]) == 3
    # dense batch
    dense = torch.cat([sts[0]] * 2)
    a0 = args(wins[0])
    ba.BA(0, dense, None, np.concatenate([a0[0]] * 2), np.concatenate([a0[1]] * 2), np.concatenate([a0[2]] * 2), a0[3], a0[4],
          np.concatenate([a0[5]] * 2), a0[6], 1e-3, 1e-3, [1e-4, 1e-4], None, initialize=True)
    cd = ba.covariance()
    assert tuple(cd.shape) == (2, sts[0].shape[1], 9, 9) and torch.equal(cd[0], cd[1])
    ba.release()
    # streaming driver: one block per batch, errors / times bitwise as without the list
    det, orb = synth.make_two_pass_sequence()
    e0, f0, t0 = od_pipe.streaming_version(det, orb)
    ba.release()
    covs = []
    e1, f1, t1 = od_pipe.streaming_version(det, orb, covariances=covs)
    assert torch.equal(e0, e1) and f0 == f1 and all(np.array_equal(a, b) for a, b in zip(t0, t1))
    assert len(covs) >= 1 and all(tuple(c.shape) == (9, 9) for c in covs)
    ba.release()


@pytest.mark.parametrize("cfg", ["C2", "C3"])
def test_sequential_and_partitioned_paths_agree(cfg):
    """The query follows the solver setting: chunk 0 = the sequential walk, chunks of 8 / 12 and two-level partitions = the partitioned
    path (chunk elimination, separator system, correction).  All agree to 1e-10 per pose, undamped and damped."""
    win = _win(cfg)
    eng = _engine(win)
    st, lam = _scheduled(win, eng)
    n = st.shape[0]
    res = {}
    for sv in (0, 8, 12, (8, 4), (12, -1)):
        if isinstance(sv, tuple):
            eng.set_solver(*sv)
        else:
            eng.set_solver(sv)
        assert eng.mode()[1] == (sv[0] if isinstance(sv, tuple) else sv)
        res[sv] = [eng.covariance(19, damped=d, super_diagonal=True) for d in (False, True)]
        for d, s, f in res[sv]:
            assert f[0] & (ZERO_PIVOT | INDEFINITE) == 0
            assert np.array_equal(d[0, :n], d[0, :n].transpose(0, 2, 1))
            assert not s[0, n - 1].any()
    for sv in (8, 12, (8, 4), (12, -1)):
        for (d0, s0, _), (d1, s1, _) in zip(res[0], res[sv]):
            assert C.block_rel_err(d1[0, :n], d0[0, :n]) < 1e-10, sv
            assert C.block_rel_err(s1[0, :n - 1], s0[0, :n - 1]) < 1e-10, sv
    eng.close()


def test_streaming_batched_collects_one_block_per_live_sequence_and_round():
    """Two sequences of different lengths: one entry per sequence per round while it has a batch, results bitwise as without the list."""
    import torch
    from vinsat_amd import ba, od_pipe, synth
    seqs = [synth.make_two_pass_sequence(), synth.make_sequence("C1")]
    ref = od_pipe.streaming_batched(seqs)
    ba.release()
    covs = []
    got = od_pipe.streaming_batched(seqs, covariances=covs)
    ba.release()
    for (e0, f0, t0), (e1, f1, t1) in zip(ref, got):
        assert torch.equal(e0, e1) and f0 == f1 and all(np.array_equal(a, b) for a, b in zip(t0, t1))
    rounds = {}
    for c in covs:
        assert tuple(c["cov"].shape) == (9, 9) and np.isfinite(c["cov"].numpy()).all()
        rounds.setdefault(c["round"], []).append(c["sequence"])
    assert all(sorted(v) == sorted(set(v)) for v in rounds.values())
    assert rounds[0] == [0, 1]
    assert len(covs) == sum(len(v) for v in rounds.values())
