"""Both paths of the covariance query (csrc/vba_cov.hip: the sequential walk k_cov_seq and the partitioned k_cov_chunk / k_cov_sep /
k_cov_fix; both run the one recurrence of csrc/vba_cov_walk.h), per component, against the system the query inverted.

Every case (tests/cov_cases.py): pipeline off, upload, states at the initial guess with lamda 1e-4, vba_step(9, landmark-only),
vba_step(10, full), then vba_covariance(14, damped, with the super-diagonal) undamped and damped, then vba_step(14, full) and its
VBA_DBG_BANDS -- the system the query inverted; the damping is float32 of the resident lamda the query met (equal to the
scalars' lamda32 whenever call 14 took one trial, asserted).  Every window is judged by tests/cov_reference.py: the scaled
componentwise error against the longdouble selected inverse of its own fetched bands, per pose and group pair, under

    bar[group] = max(M * max(error[group] of the four fp64 CPU references on that same system), M * 2^-52),   M = 16

-- the factor of tests/test_gpu_solve_paths.py for the unpivoted paths, whose reasoning carries over (the same elimination step,
another order of the same block eliminations); the fourth reference is the partitioned algorithm at the case's chunk size, so the
bar carries that method's own rounding.  No bar comes from a device run; tests/test_cov_reference_host.py plants the faults that
must exceed these bars.  Also per window: no ZERO_PIVOT / INDEFINITE, diagonal blocks bitwise symmetric, super[n - 1] zero, and
zeros in the rows beyond n of a loose or ragged handle, in diag and super (include/vinsat_ba.h promises both; for diag the
header said nothing before, both paths already wrote zeros there, and the promise was added).

Largest measured device / CPU ratios on the MI355X (figure / max(CPU figure of the group, 2^-52); the bar is at 16):

  test_sequential_walk    1.69 (n = 2, undamped, super vel-att)
  test_partitioned        1.72 (chunk 3, n = 4, tight handle, undamped, super pos-pos pose 1); tight and loose handles alike
  test_batches            3.22 (chunks of 2, latency kernels, the two-pose window, damped, super vel-att); 2.33 with chunks of 5

No case exposed a fault in csrc/vba_cov.hip or csrc/vba_cov_walk.h.
"""
import numpy as np
import pytest

import cov_cases as K
import cov_reference as R

pytestmark = pytest.mark.gpu

M = 16
RATIOS = {}


def engine(n_max, windows=1, mode=-1):
    from vinsat_amd.engine import BAEngine
    e = BAEngine(n_max, K.ROWS * n_max, windows=windows, mode=mode)
    e.set_pipeline(False)
    return e


def upload(e, w, k=0):
    win, t, st0 = w
    e.upload_observations(win.landmarks_xyz, win.landmarks_uv, win.confidences, win.ii, t.size, window=k)
    e.upload_window(win.intrinsics, win.cumrot_last, t, window=k)
    e.set_states(st0, 1e-4, window=k)


def query(e, wins, who, where, s_ref, stepped=True):
    """Run the case on ``e`` (``stepped`` False: the states are already resident) and judge every window.  Returns
    (list of what is out of bounds, {damped: (diag, super, flags)})."""
    W, bad = len(wins), []
    if stepped:
        for k, w in enumerate(wins):
            upload(e, w, k)
        for it, init in K.SCHEDULE:
            e.step(it, init)
    res = {d: e.covariance(K.QUERY_ITER, damped=d, super_diagonal=True) for d in (False, True)}
    lams = [e.get_states(window=k)[1] for k in range(W)]
    e.step(K.QUERY_ITER, False)
    for k, w in enumerate(wins):
        n = w[1].size
        bands, sc = e.debug("bands", window=k), e.debug("scalars", window=k)
        lam32 = float(np.float32(lams[k]))
        if sc[7] == 1:
            assert sc[4] == lam32, (where, k, sc[4], lam32)
        for d in (False, True):
            diag, sup, flags = res[d]
            at = f"{where} n={n} w={k} {'damped' if d else 'undamped'}"
            if flags[k] & (R.ZERO_PIVOT | R.INDEFINITE):
                bad.append(f"{at}: flags {flags[k]}")
                continue
            lv = R.levels(bands, lam32 if d else 0.0, s_ref if s_ref else n)
            v = R.judge(diag[k, :n], sup[k, :n], lv, M)
            r = RATIOS.setdefault(who, [0.0, None])
            if v.ratio > r[0]:
                r[0], r[1] = v.ratio, f"{at}, {v.ratio_at}"
            bad += [f"{at}: {b}" for b in v.bad]
            if not np.array_equal(diag[k, :n], diag[k, :n].transpose(0, 2, 1)):
                bad.append(f"{at}: a diagonal block is not bitwise symmetric")
            if sup[k, n - 1].any():
                bad.append(f"{at}: super[n - 1] is not zero")
            if diag[k, n:].any() or sup[k, n:].any():
                bad.append(f"{at}: rows beyond n are not zero")
    return bad, res


def report(who, bad):
    r = RATIOS.get(who)
    if r:
        print(f"\n{who}: largest device / CPU ratio {r[0]:.3g} ({r[1]})")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("n", K.SEQUENTIAL)
def test_sequential_walk(n):
    who = "test_sequential_walk"
    e = engine(n)
    e.set_solver(0)
    assert e.mode()[1] == 0
    bad, _ = query(e, [K.window(n)], who, "walk", 0)
    e.close()
    report(who, bad)


@pytest.mark.parametrize("loose", [False, True], ids=["tight", "loose"])
@pytest.mark.parametrize("s", sorted(K.CHUNKED))
def test_partitioned(s, loose):
    who, bad = "test_partitioned", []
    for n in K.CHUNKED[s]:
        e = engine(K.loose_n_max(n) if loose else n)
        e.set_solver(s)
        assert e.mode()[1] == s
        bad += query(e, [K.window(n)], who, f"chunk {s} n_max {e.n_max}", s)[0]
        e.close()
    report(who, bad)


def test_second_level_settings_do_not_reach_the_query():
    """The partitioned covariance reads the first-level chunk only: (5, 4) and (5, -1) give the bits of (5)."""
    n, got = 33, []
    for sv in ((5,), (5, 4), (5, -1)):
        e = engine(n)
        e.set_solver(5)
        w = K.window(n)
        upload(e, w)
        for it, init in K.SCHEDULE:
            e.step(it, init)
        e.set_solver(*sv)
        got.append([e.covariance(K.QUERY_ITER, damped=d, super_diagonal=True) for d in (False, True)])
        e.close()
    for other in got[1:]:
        for (d0, s0, f0), (d1, s1, f1) in zip(got[0], other):
            assert np.array_equal(d0, d1) and np.array_equal(s0, s1) and f0[0] == f1[0]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("s,n_max,solver", [(5, 16, 5), (2, 9, 2), (5, 16, 0)])
def test_batches(s, n_max, solver, mode):
    """Five windows of (n_max, s + 1, s, 2, 2 s - 1) poses on one handle: each against its own reference, and with the bits of the
    same window alone (its states taken from the batch) on a handle of the same n_max, solver setting and kernel set."""
    who = "test_batches"
    wins = K.batch_windows(s, n_max)
    e = engine(n_max, windows=5, mode=mode)
    e.set_solver(solver)
    assert e.mode() == (mode, solver)
    for k, w in enumerate(wins):
        upload(e, w, k)
    for it, init in K.SCHEDULE:
        e.step(it, init)
    S, lams = e.get_states_all()[:2]
    bad, res = query(e, wins, who, f"batch chunk {solver} mode {mode}", solver, stepped=False)
    e.close()
    for k, w in enumerate(wins):
        n = w[1].size
        one = engine(n_max, mode=mode)
        one.set_solver(solver)
        assert one.mode() == (mode, solver)
        upload(one, w)
        one.set_states(S[k, :n], lams[k])
        for d in (False, True):
            d1, s1, f1 = one.covariance(K.QUERY_ITER, damped=d, super_diagonal=True)
            if not (np.array_equal(d1[0], res[d][0][k]) and np.array_equal(s1[0], res[d][1][k]) and f1[0] == res[d][2][k]):
                bad.append(f"batch chunk {solver} mode {mode} w={k} n={n}: not the bits of the window alone")
        one.close()
    report(who, bad)
