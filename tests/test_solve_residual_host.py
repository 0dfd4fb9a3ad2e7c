"""The residual judge of tests/solve_residual.py on the recorded systems (no GPU, no library): reference levels of the three CPU
solves, and the proof that the bars of tests/test_gpu_solve_paths.py can fail -- planted faults must exceed them.

Systems: every ``A_bands_k`` / ``JTr_k`` / ``dpose_k`` of tests/golden/{c1,c2,rej,gap}.npz (c1: 20 calls, c2: 4, rej: 4 calls with
2 .. 9 trials each; gap records none), 45 in all.

Reference levels measured here (max over the three CPU solves): omega 2e-15 .. 9e-13 on c1 and c2, up to 8e-12 on rej call 16;
forward error up to 4e-8 (c1 call 10, condition ~1e14).  The two pivoted LUs set them: the unpivoted block recurrence alone
stays at 2e-16 .. 3e-14 in omega on every recorded system.

Planted faults (M = 16, bars formed as the GPU test forms them), measured on c2 call 10 / c1 call 10:
  (a) component 0 of pose n/2 times 1 + 1e-8: omega 1.5e-10 / 5.7e-10 against bars of 5.0e-12 / 1.3e-12.  The smallest planted
      relative error the omega bar still catches at that component of c2 call 10 is 3e-10; over all 882 (interior pose, component)
      pairs of c2 call 10 it is 2.7e-9 for the least sensitive pair (1e-8 is caught at every pair, 1e-9 at 875 of 882).  The
      forward bar does not see (a) at all (1e-8 is below the CPU solves' own forward error): the residual is what sharpens.
      Against the wider omega bar of the pivoted kernels (M_PIVOTED = 214: 6.7e-11 / 1.7e-11) the smallest caught is 4.5e-9.
  (b) pose n/2 replaced by its neighbour: omega ~1.
  (c) damping left off one diagonal block: 1e-4 against diagonal entries of 2e6 .. 2e10, a relative change of 5e-11 .. 5e-15.
      Over the 100 blocks of c2 this fault measures 6.5 .. 95 times the CPU level in omega and 13 .. 650 times in forward error:
      above a bar of 16 at 99 blocks, under both at pose 20.  So this fault is at the edge of what the bars resolve, and which
      blocks show it depends on how LAPACK rounds the solve that sets the CPU level (pose 88 of c2: 65 times in omega with the
      factors kept for the refinement, 78 with np.linalg.solve).
      The test plants it where the forward error leaves a wide margin on any build -- pose 88 of c2 (565 times the CPU level)
      and pose 3 of c1 (830) -- and asserts what holds there: the forward bar is exceeded, M = 16 and M_PIVOTED_FWD = 84 alike.
      Its omega is printed, not asserted.
  (d) the chain ended one pose early, two readings: pose n-2 takes the value it has in the system truncated after it; and the
      whole truncated solve with the last pose kept.  omega 0.1 .. 0.7."""
import numpy as np
import pytest

from conftest import load_golden
import solve_residual as S

DPOSE_TOL = 1e-7            # tests/test_gpu_parity.py
M = 16                      # tests/test_gpu_solve_paths.py: the unpivoted kernels
M_PIVOTED = 214             # ... and the pivoted ones, omega (Gauss-Jordan with row exchanges; that module's docstring has the reason)
M_PIVOTED_FWD = 84          # ... and forward error


def _systems(name):
    g = load_golden(name)
    for key in sorted((k for k in g.files if k.startswith("A_bands_")), key=lambda s: int(s.split("_")[-1])):
        k = int(key.split("_")[-1])
        A, b, d = g[key], g[f"JTr_{k}"], g[f"dpose_{k}"]
        n = A.shape[1]
        for t in range(A.shape[0]):
            yield k, t, A[t], b[t].reshape(n, 9), d[t].reshape(n, 9)


@pytest.fixture(scope="module")
def recorded():
    """[(fixture, call, trial, damped bands, rhs, recorded dpose, Levels)] of every recorded system, computed once."""
    out = []
    for name in ("c1", "c2", "rej", "gap"):
        for k, t, A, b, d in _systems(name):
            out.append((name, k, t, A, b, d, S.levels(A, b)))
    return out


def test_cpu_solves_agree_with_the_recorded_dpose(recorded):
    assert len(recorded) >= 45
    for name, k, t, A, b, d, lv in recorded:
        for how, x in lv.solves.items():
            assert np.abs(x - d).max() / np.abs(d).max() < DPOSE_TOL, (name, k, t, how)


def test_reference_levels(recorded):
    """The worst of the three CPU solves per fixture, printed, and asserted: omega <= 5e-11 -- the reference's own error, 8e-12 at
    its worst (rej call 16, last trial: damping 1e4 beside entries of 2e10), with headroom for another LAPACK build; planted
    fault (a) at 1.5e-10 would not pass as a reference level.  The unpivoted recurrence alone stays within 9n 2^-52 (no row
    exchanges, no scale mixing); the forward error stays within the bar the recorded dpose is held to."""
    worst = {}
    for name, k, t, A, b, d, lv in recorded:
        w = worst.setdefault(name, dict(omega=0.0, at=None, dp=0.0, dtheta=0.0, dv=0.0))
        if lv.omega > w["omega"]:
            w["omega"], w["at"] = lv.omega, (k, t)
        for grp in ("dp", "dtheta", "dv"):
            w[grp] = max(w[grp], lv.fwd[grp])
        n = A.shape[0]
        assert lv.omega <= 5e-11, (name, k, t, lv.omega)
        assert all(v <= DPOSE_TOL for v in lv.fwd.values()), (name, k, t, lv.fwd)
        own = S.omega(A, lv.solves["thomas"], b).value
        assert own <= 9 * n * S.EPS, (name, k, t, own)         # no row exchanges: no scale mixing
    for name, w in worst.items():
        print(f"reference levels {name}: omega {w['omega']:.2e} at call/trial {w['at']}, forward dp {w['dp']:.2e} "
              f"dtheta {w['dtheta']:.2e} dv {w['dv']:.2e}")


def _planted(A, b, x0, lam32, eps, pose_c):
    n = A.shape[0]
    i = n // 2
    out = {}
    x = x0.copy()
    x[i, 0] *= 1.0 + eps
    out["a: one component times 1 + %g" % eps] = x
    x = x0.copy()
    x[i] = x0[i + 1]
    out["b: a pose replaced by its neighbour"] = x
    A2 = A.copy()
    A2[pose_c, 1] -= lam32 * np.eye(9)
    out["c: damping left off one diagonal block"] = np.linalg.solve(S.dense_from_bands(A2), b.reshape(-1)).reshape(n, 9)
    xt = np.linalg.solve(S.dense_from_bands(A[:n - 1]), b[:n - 1].reshape(-1)).reshape(n - 1, 9)
    x = x0.copy()
    x[n - 2] = xt[n - 2]
    out["d: pose n-2 as if the chain ended there"] = x
    x = x0.copy()
    x[:n - 1] = xt
    out["d: the chain solved without its last pose"] = x
    return out


@pytest.mark.parametrize("name,k,pose_c", [("c2", 10, 88), ("c1", 10, 3)])
def test_planted_faults_exceed_the_gpu_bars(name, k, pose_c):
    """Every planted fault fails the check of the unpivoted kernels (M) and that of the pivoted ones (M_PIVOTED, M_PIVOTED_FWD)."""
    g = load_golden(name)
    _, _, A, b, _ = next(s for s in _systems(name) if s[0] == k)
    lam32 = float(np.float32(g["lamda_in"][k]))
    lv = S.levels(A, b)
    x0 = lv.solves["dense"]
    clean = S.judge(A, x0, b, M, lv)
    assert clean.ok                                             # the unplanted solution passes
    print(f"{name} call {k}: bar omega {lv.bar_omega(M):.2e}, bar forward {({q: '%.1e' % v for q, v in lv.bar_fwd(M).items()})}")
    for what, x in _planted(A, b, x0, lam32, 1e-8, pose_c).items():
        v = S.judge(A, x, b, M, lv)
        print(f"  {what}: omega {v.omega.value:.2e} at pose {v.omega.worst_pose} ({v.ratio_omega:.3g} x CPU), forward "
              f"{({q: '%.1e' % e for q, e in v.fwd.items()})} ({v.ratio_fwd:.3g} x CPU)")
        assert not v.ok and not S.judge(A, x, b, M_PIVOTED, lv, M_fwd=M_PIVOTED_FWD).ok, (name, what)
        if what.startswith("c"):            # a change of 5e-11 .. 5e-15 of the diagonal: the forward bars see it (module docstring)
            assert any(v.fwd[q] > max(M, M_PIVOTED_FWD) * lv.fwd[q] for q in v.fwd), (name, what, v.fwd)
        else:
            assert v.omega.value > lv.bar_omega(M_PIVOTED) > lv.bar_omega(M), (name, what, v.omega.value)
        if what[0] in "bd":                 # the pose named by the per-pose figure is the planted one or its neighbour
            n = A.shape[0]
            assert abs(v.omega.worst_pose - (n // 2 if what[0] == "b" else n - 2)) <= 1, (what, v.omega.worst_pose)


def test_landmark_only_call_has_rows_without_denominator():
    """c1 call 0: block diagonal, the velocity slots carry the damping alone and a zero right-hand side -- 3 n rows whose
    denominator vanishes.  They are found, their residual is exactly 0 and they stay out of omega; a non-zero value planted in
    one of them is reported as a residual on a zero-denominator row."""
    _, _, A, b, d = next(s for s in _systems("c1") if s[0] == 0)
    n = A.shape[0]
    lv = S.levels(A, b)
    for how, x in lv.solves.items():
        om = S.omega(A, x, b)
        assert om.zero_rows.sum() == 3 * n and om.zero_rows[:, 6:].all(), how
        assert om.zero_rows_residual == 0.0 and np.isfinite(om.value) and np.isfinite(om.per_pose).all(), how
        assert S.forward_err(x, lv.xs)["dv"] == 0.0
    x = lv.solves["dense"].copy()
    x[4, 7] = 1e-30
    v = S.judge(A, x, b, M, lv)
    assert not v.ok and v.fwd["dv"] == float("inf")
    x[4, 7] = np.nan
    assert not S.judge(A, x, b, M, lv).ok
