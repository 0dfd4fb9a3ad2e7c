"""Every block-tridiagonal solve path against the system it solved.

After a ``vba_step`` the library hands out the undamped bands, the right-hand side, the fp32 damping of the last trial and the step
the device computed (``vba_debug_fetch``).  ``check`` below judges that step by its componentwise backward error ``omega`` in
extended precision and by its forward error per slot group (tests/solve_residual.py), against bars formed from three fp64 CPU
solves of THAT SAME fetched system:

    bar_omega = max(M * max(omega of the CPU solves), M * 2^-52),    bar_fwd[group] = M * max(forward_err of the CPU solves)

``M = 16`` for the unpivoted kernels (the default path): cyclic reduction puts up to seven levels of block eliminations on top of
the chain's and the two-sided chunks use another elimination order, while the unpivoted device paths are recorded as closer to the
reference than LAPACK's banded LU (header of test_gpu_parity.py) -- 16 times the worst CPU solve is generous for
rounding and four to five orders below what a wrong block gives (tests/test_solve_residual_host.py plants the faults and proves
it).  Measured: every unpivoted path stays below 11 in omega and below 10 in forward error (table below).  No bar comes from a
device run.

``M_PIVOTED = 214`` (omega) and ``M_PIVOTED_FWD = 84`` (forward error) for the pivoted kernels (``vba_set_pivoting``; the
fallback of the default path).  They were meant to share M = 16 and do not reach it: measured 3 .. 107 times the CPU level in omega (the largest: the landmark-only call 9 of window 7 of
test_default_rule_18_windows, pose 9, omega 7.2e-13 against 6.7e-15 of the CPU solves) and up to 42 in forward error
(test_mixed_handle, 50 poses, call 14).  The cause is the method, not an index: ``forward_step<PIVOT = true>`` (vba_solve_step.h)
is Gauss-Jordan elimination with row exchanges inside the 9x9 block.  Gauss-Jordan is backward stable for the (nearly) symmetric
positive definite blocks the unpivoted path meets, but in general its residual carries the condition of the triangular factor
on top of Gaussian elimination's (Higham, Accuracy and Stability of Numerical Algorithms, Theorem 14.5), and a row exchange
between a position row (diagonal ~2e6) and a rotation or velocity row (~2e9 .. 2e10) is what makes that factor ill conditioned.
The same arithmetic in NumPy on the recorded landmark-only blocks of c2 call 9 gives omega 1.4e-12 with row exchanges, 9.9e-16
without and 1.5e-13 for LAPACK's LU: the figure belongs to the algorithm, on the CPU as on the device, every pivoted kernel
shares that step, and no path stands out (sequential 12, chunks 18, one workgroup 34, split levels 78, landmark-only 107).
Rewriting the fallback as elimination plus back substitution is not a test's business.  The rule for a correct path that needs
more than 16 is followed instead: no silent raise -- the kernel read, the largest ratio and its case recorded, and the factor set
to twice that ratio, for omega (2 x 107) and for the forward error (2 x 42) each from its own measurement.  Every planted fault of
the host test exceeds these bars as well: (a), (b) and (d) in omega, (c) in forward error.

In latency mode the bands are re-formed by the assembly at fetch time while the chunk kernel formed its own blocks in LDS, so the
residual there also checks the fused forming against the assembled system.

Every case runs [(9, landmark-only), (10, full), (14, full)] from the initial guess with lamda 1e-4 through ``vba_step`` and is
checked after each call; flags == 0; unpivoted cases assert that no solve fell back to the pivoted kernels.  Windows: synthetic,
3 rows per pose (tests/solve_residual.py ``window_for``).

Where each case lands (launch_solve_variant, vba_solve.hip; launch_chunks_t, vba_solve_chunks.hip; launch_cr_front2 /
launch_cr_short, vba_solve_cr.hip; launch_walk_t, vba_solve_seq.hip).  Call 9 of every case: k_solve_blockdiag, or in latency mode
on the unpivoted path the 6x6 solve inside the trial kernel (fused_trial 1).  Calls 10 and 14, "sep" = ceil(n / chunk) - 1:

  test_sequential_walk               chunk 0, one window: k_solve (set_solver(0) and (-2) alike with one window)
  test_four_windows_per_wave         chunk 0, bandwidth mode: W = 1 -> k_solve; W >= 2 -> k_solve_quad<., forms> (fusion bit 2 on by
                                     default), groups of four with a partial last group for W = 3, 5, 9; pose counts differ in a wave
  test_one_level_chunks              chunks of 2, 5, 8, chunk2 = 0: k_solve_chunks_ts_fused (chunk >= 4) or k_solve_chunks_fused
                                     (chunk 2), then k_solve_reduced walking 0 .. 7 separators, recovery in the trial kernel
  test_chunk_waves                   chunks of 4, 5 with cyclic reduction; latency mode: k_solve_chunks_fused (waves 1) /
                                     k_solve_chunks_ts_fused (waves 2); bandwidth mode: k_solve_chunks / k_solve_chunks_ts + k_solve_recover;
                                     last chunks of 1 (n = kc + 1: the two-sided kernel falls back to one wave below 3 poses), c - 1 and c
                                     poses; 0 .. 7 separators -> k_solve_reduced_cr<., 0>
  test_cyclic_reduction_in_workgroup chunks of 2, separators 1 .. 23 -> k_solve_reduced_cr<., 0> (below kCrSplitMin = 24); handle of
                                     48 poses, so the one-workgroup kernel is sized for 23 blocks throughout ...
  test_cyclic_reduction_tight_handle ... and with n_max = n at 1, 2, 3 and 23 separators (both parities of n): launch_cr_short sizes the
                                     LDS (nb * 252 doubles) and the chunk grid from n_max, so these are the tight allocations
  test_split_cyclic_reduction        chunks of 2, separators 24 .. 128 -> k_cr_level01 (four separators per block: 24 .. 28 cover every
                                     residue) + k_solve_reduced_cr<., 2>; chunks of 3 at n = 100 (33) and of 8 at n = 200 (24)
  test_mixed_handle                  (100, 60, 20) poses, chunks of 3: 33 / 19 / 6 separators; (50, 48, 6) poses, chunks of 2: 24 / 23 / 2 --
                                     one launch each of k_cr_level01 + tail and of the one-workgroup kernel, every window taken by one
  test_two_levels                    (3, 2), (5, 4), (4, 3): chunk kernel + k_solve_chunks2 + k_solve_reduced + k_solve_recover2, ragged
                                     first level, ragged second level, both
  test_fused_forming_limit           latency mode, chunks of 28 (kFusedChunkMax: k_solve_chunks_ts_fused with mask 15) and 29
                                     (k_solve_chunks_ts behind the assembly); mask 12: the assembled path for both
  test_default_rule                  set_solver(-1): n < 8 -> k_solve; latency mode chunks of min(8, n / 3), bandwidth mode of
                                     min(12, n / 3), cyclic reduction; 18 windows of 64 poses (windows 0, 7, 17 fetched)
  test_ba_reg                        vba_set_prior(1): the REG instantiations of the forming chunk kernel; 12 (one workgroup) and
                                     24 (split) separators
  test_long_gap_window               26 poses, gaps of 1 .. 60 s and two of 700 s, chunks of 2 (12 separators)
  test_comparison_solvers            comparison build only (launch_comparison_t, vba_solve_variants.hip): k_solve_packed (five windows of 47 / 100
                                     poses); fusion bit 4 with chunks of 2: n = 100 (49 separators) -> k_cr_level0 + k_solve_reduced_cr<., 1>,
                                     n = 47 (23) -> the one-workgroup kernel through that dispatch; fusion bits 5 / 6 -> k_solve_resident, which
                                     needs chunks >= 4 and >= 24 separators: n = 100 with chunks of 4 and n = 200 with chunks of 8 (24 each)
  test_packed_walk_pivoted_fallback  comparison build only: k_solve_packed<false> hands a window to k_solve_packed<true> within a call

Largest measured device / CPU ratios on the MI355X (omega against max(omega_cpu, 2^-52); forward error against the CPU
solves'), per test function (unpivoted: M = 16, pivoted: M_PIVOTED = 214 / M_PIVOTED_FWD = 84):

  test_sequential_walk                 unpivoted omega 0.74, forward 4.7   | pivoted omega 11.6 (n=65 call 9),  forward 5.8
  test_four_windows_per_wave           unpivoted omega 1.4,  forward 2.8   | pivoted omega 3.7,               forward 13.7 (W=5, n=3, call 14)
  test_one_level_chunks                unpivoted omega 2.0,  forward 4.7   | pivoted omega 17.5 (chunk 5 n=36 call 14), forward 30.6 (same)
  test_chunk_waves                     unpivoted omega 2.0,  forward 5.0   | pivoted omega 16.6 (chunk 5 n=36 call 14), forward 27.6 (same)
  test_cyclic_reduction_in_workgroup   unpivoted omega 10.2 (5 separators, call 9), forward 3.4 | pivoted omega 34.4 (23 separators, n=47), forward 21.8
  test_cyclic_reduction_tight_handle   unpivoted omega 0.63, forward 3.4   | pivoted omega 34.4 (23 separators, n=47), forward 21.8
  test_split_cyclic_reduction          unpivoted omega 2.1,  forward 6.6 (63 separators) | pivoted omega 78.2 (chunk 3, 33 separators, call 14), forward 16.3
  test_mixed_handle                    unpivoted omega 0.99, forward 1.7   | pivoted omega 22.2 (n=48), forward 42.3 (n=50 call 14)
  test_two_levels                      unpivoted omega 10.2 (4/3, n=12, call 9), forward 3.2 | pivoted omega 10.6, forward 22.4 (4/3, n=37)
  test_fused_forming_limit             unpivoted omega 0.74, forward 1.0   | pivoted omega 40.3 (chunk 28 n=59 call 14), forward 9.9
  test_default_rule (both functions)   unpivoted omega 2.1,  forward 3.4   | pivoted omega 107 (W=18, window 7, call 9), forward 14.2
  test_ba_reg                          unpivoted omega 1.9,  forward 1.5   | pivoted omega 2.7,  forward 1.4
  test_long_gap_window                 unpivoted omega 0.06, forward 0.15  | pivoted omega 3.6,  forward 2.0
  test_comparison_solvers              unpivoted omega 2.1 (resident, chunk 8, n=200), forward 5.2 (packed, n=47) | pivoted omega 49.5 (one level in front, n=100), forward 12.8 (resident, chunk 4, n=100)
  test_packed_walk_pivoted_fallback    omega 0.45, forward 2.0 (judged by the pivoted bars)

(The unpivoted figures of 10 belong to landmark-only calls of short windows, where the CPU level is the 2^-52 floor.)
The packed walk of the comparison build used to answer a window that needs the pivoted fallback with "LM loop did not terminate
within 24 trials": it raised the flag that asks the host for the pivoted repeat but not the one that hands the window to the
pivoted kernels, so the repeat turned the window away.  Fixed in k_solve_packed; test_packed_walk_pivoted_fallback runs the five
47-pose windows that showed it (the one of seed 300 falls back at call 14).
"""
import numpy as np
import pytest

import solve_residual as S

pytestmark = pytest.mark.gpu

M = 16
M_PIVOTED = 214
M_PIVOTED_FWD = 84
SCHEDULE = [(9, True), (10, False), (14, False)]
PIVOT = pytest.mark.parametrize("pivot", [False, True], ids=["unpivoted", "pivoted"])

_WINDOWS = {}
RATIOS = {}             # (test function, pivoted) -> [largest omega ratio, largest forward ratio, where, where]
# window(57) with its own seed sends the unpivoted path of call 14 to the pivoted kernels (a rejected trial at high damping):
# another seed for that pose count
SEEDS = {57: 1057}


def window(n, seed=None, rows=3, gaps=None):
    """(win, time_idx, states0) of ``n`` poses, made once per session and left unchanged."""
    seed = SEEDS.get(n, n) if seed is None else seed
    key = (n, seed, rows, None if gaps is None else tuple(int(g) for g in gaps))
    if key not in _WINDOWS:
        _WINDOWS[key] = S.window_for(n, rows, seed, gaps)
    return _WINDOWS[key]


def engine(n_max, windows=1, mode=-1, rows=3):
    from vinsat_amd.engine import BAEngine
    return BAEngine(n_max, rows * n_max, windows=windows, mode=mode)


def upload(e, w, k=0):
    win, t, st0 = w
    e.upload_observations(win.landmarks_xyz, win.landmarks_uv, win.confidences, win.ii, t.size, window=k)
    e.upload_window(win.intrinsics, win.cumrot_last, t, window=k)
    e.set_states(st0, 1e-4, window=k)


def check(e, k, who, where, chunk=0):
    """Window ``k`` of the call that ran last: [] or the list of what is out of bounds."""
    bands, rhs, dpose = e.debug("bands", window=k), e.debug("rhs", window=k), e.debug("dpose", window=k)
    A = S.damped(bands, e.debug("scalars", window=k)[4])
    v = S.judge(A, dpose, rhs, M_PIVOTED, M_fwd=M_PIVOTED_FWD) if who[1] else S.judge(A, dpose, rhs, M)
    r = RATIOS.setdefault(who, [0.0, 0.0, None, None])
    if v.ratio_omega > r[0]:
        r[0], r[2] = v.ratio_omega, where
    if v.ratio_fwd > r[1]:
        r[1], r[3] = v.ratio_fwd, where
    bad = []
    flags = e.get_states(window=k)[4]
    if flags != 0:
        bad.append(f"{where}: flags {flags}")
    if v.omega.zero_rows_residual != 0.0:
        bad.append(f"{where}: residual {v.omega.zero_rows_residual:.3e} on a row without denominator")
    if not v.omega.value <= v.bar_omega:
        p = v.omega.worst_pose
        bad.append(f"{where}: omega {v.omega.value:.3e} > {v.bar_omega:.3e} ({v.ratio_omega:.3g} x CPU) at pose {p} of {A.shape[0]}"
                   + (f", chunk {p // chunk} offset {p % chunk}" if chunk > 0 else ""))
    for g in v.fwd:
        if not v.fwd[g] <= v.bar_fwd[g]:
            bad.append(f"{where}: forward error of {g} {v.fwd[g]:.3e} > {v.bar_fwd[g]:.3e}")
    return bad


def run(e, wins, who, where, pivot, chunk=0, fetch=None, prior=None, falls_back=False):
    """Upload ``wins`` into the windows of ``e``, run the schedule and check the fetched windows after every call.
    ``falls_back``: an unpivoted handle some window of which must reach the pivoted kernels (judged by their bars: pivot = True)."""
    who = (who, pivot)
    for k, w in enumerate(wins):
        upload(e, w, k)
    if prior is not None:
        e.upload_prior(*prior)
        e.set_prior(True)
    before = e.solver_fallbacks()
    bad = []
    for it, init in SCHEDULE:
        e.step(it, init)
        for k in (range(len(wins)) if fetch is None else fetch):
            bad += check(e, k, who, f"{where} n={wins[k][1].size} w={k} call {it}", chunk)
    if falls_back and e.solver_fallbacks() == before:
        bad.append(f"{where}: no window fell back to the pivoted kernels")
    if not pivot and not falls_back and e.solver_fallbacks() != before:
        bad.append(f"{where} n={[w[1].size for w in wins]}: the unpivoted path fell back to the pivoted kernels")
    return bad


def report(who, bad, pivot):
    r = RATIOS.get((who, pivot))
    if r:
        print(f"\n{who} {'pivoted' if pivot else 'unpivoted'}: largest omega ratio {r[0]:.3g} ({r[2]}), largest forward ratio {r[1]:.3g} ({r[3]})")
    assert not bad, "\n".join(bad)


def sweep(c):
    return sorted({n for n in (c - 1, c, c + 1, 2 * c, 2 * c + 1, 3 * c - 1, 7 * c + 1) if n >= 2})


# ---------------------------------------------------------------------------------------------------------------- sequential
@PIVOT
@pytest.mark.parametrize("solver", [0, -2])
def test_sequential_walk(solver, pivot):
    who, bad = "test_sequential_walk", []
    e = engine(65)
    e.set_solver(solver)
    e.set_pivoting(pivot)
    for n in (2, 3, 4, 9, 65):
        bad += run(e, [window(n)], who, f"solver {solver}", pivot)
    e.close()
    report(who, bad, pivot)


@PIVOT
@pytest.mark.parametrize("W", [1, 3, 4, 5, 9])
def test_four_windows_per_wave(W, pivot):
    who = "test_four_windows_per_wave"
    ns = (2, 17, 9, 16, 3, 17, 5, 11, 4)[:W]
    e = engine(17, windows=W, mode=0)
    e.set_solver(0)
    e.set_pivoting(pivot)
    bad = run(e, [window(n, seed=100 + k) for k, n in enumerate(ns)], who, f"W={W}", pivot)
    e.close()
    report(who, bad, pivot)


# ---------------------------------------------------------------------------------------------------------------- chunks
@PIVOT
@pytest.mark.parametrize("c", [2, 5, 8])
def test_one_level_chunks(c, pivot):
    who, bad = "test_one_level_chunks", []
    e = engine(7 * c + 1)
    e.set_solver(c, 0)
    e.set_pivoting(pivot)
    for n in sweep(c):
        bad += run(e, [window(n)], who, f"chunk {c}", pivot, chunk=c)
    e.close()
    report(who, bad, pivot)


@PIVOT
@pytest.mark.parametrize("mode", [1, 0], ids=["latency", "bandwidth"])
@pytest.mark.parametrize("waves", [1, 2])
@pytest.mark.parametrize("c", [4, 5])
def test_chunk_waves(c, waves, mode, pivot):
    who, bad = "test_chunk_waves", []
    e = engine(7 * c + 1, mode=mode)
    e.set_solver(c, -1)
    e.set_chunk_waves(waves)
    e.set_pivoting(pivot)
    for n in sweep(c):
        bad += run(e, [window(n)], who, f"chunk {c} waves {waves} mode {mode}", pivot, chunk=c)
    e.close()
    report(who, bad, pivot)


# ---------------------------------------------------------------------------------------------------------------- cyclic reduction
def _n_for(sep, odd):
    """Pose count with chunks of 2 and ``sep`` separators: even n ends in a full chunk, odd n in a chunk of one pose."""
    return 2 * sep + (1 if odd else 2)


@PIVOT
def test_cyclic_reduction_in_workgroup(pivot):
    who, bad = "test_cyclic_reduction_in_workgroup", []
    cases = [(s, False) for s in (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 22, 23)] + [(1, True), (3, True), (23, True)]
    e = engine(48)
    e.set_solver(2, -1)
    e.set_pivoting(pivot)
    for sep, odd in cases:
        n = _n_for(sep, odd)
        assert (n + 1) // 2 - 1 == sep
        bad += run(e, [window(n)], who, f"sep {sep}", pivot, chunk=2)
    e.close()
    report(who, bad, pivot)


@PIVOT
@pytest.mark.parametrize("n", [3, 4, 5, 6, 7, 8, 47, 48])
def test_cyclic_reduction_tight_handle(n, pivot):
    who = "test_cyclic_reduction_tight_handle"
    e = engine(n)
    e.set_solver(2, -1)
    e.set_pivoting(pivot)
    bad = run(e, [window(n)], who, f"n_max = n, sep {(n + 1) // 2 - 1}", pivot, chunk=2)
    e.close()
    report(who, bad, pivot)


@PIVOT
@pytest.mark.parametrize("c,n", [(2, _n_for(s, False)) for s in (24, 25, 26, 27, 28, 31, 32, 33, 63, 64, 65, 127, 128)] + [(2, 51), (3, 100), (8, 200)])
def test_split_cyclic_reduction(c, n, pivot):
    who = "test_split_cyclic_reduction"
    sep = (n + c - 1) // c - 1
    assert 24 <= sep <= 128
    e = engine(n)
    e.set_solver(c, -1)
    e.set_pivoting(pivot)
    bad = run(e, [window(n)], who, f"chunk {c} sep {sep}", pivot, chunk=c)
    e.close()
    report(who, bad, pivot)


@PIVOT
@pytest.mark.parametrize("c,ns", [(3, (100, 60, 20)), (2, (50, 48, 6))])
def test_mixed_handle(c, ns, pivot):
    who = "test_mixed_handle"
    e = engine(max(ns), windows=3)
    e.set_solver(c, -1)
    e.set_pivoting(pivot)
    bad = run(e, [window(n, seed=40 + k) for k, n in enumerate(ns)], who, f"chunk {c}", pivot, chunk=c)
    e.close()
    report(who, bad, pivot)


@PIVOT
@pytest.mark.parametrize("c,c2", [(3, 2), (5, 4), (4, 3)])
def test_two_levels(c, c2, pivot):
    who, bad = "test_two_levels", []
    p = c * c2
    ns = (p - 1, p, p + 1, 3 * p + 1, 3 * p + c + 1)
    e = engine(max(ns))
    e.set_solver(c, c2)
    e.set_pivoting(pivot)
    for n in ns:
        bad += run(e, [window(n)], who, f"chunks {c}/{c2}", pivot, chunk=c)
    e.close()
    report(who, bad, pivot)


@PIVOT
@pytest.mark.parametrize("mask", [15, 12])
@pytest.mark.parametrize("c", [28, 29])
def test_fused_forming_limit(c, mask, pivot):
    who, bad = "test_fused_forming_limit", []
    e = engine(85, mode=1)
    e.set_solver(c, -1)
    e.set_fusion(mask)
    e.set_pivoting(pivot)
    for n in (57, 59, 85):
        bad += run(e, [window(n)], who, f"chunk {c} mask {mask}", pivot, chunk=c)
    e.close()
    report(who, bad, pivot)


# ---------------------------------------------------------------------------------------------------------------- defaults
@PIVOT
@pytest.mark.parametrize("mode", [1, 0], ids=["latency", "bandwidth"])
@pytest.mark.parametrize("n", [7, 8, 23, 24, 25, 200])
def test_default_rule(n, mode, pivot):
    who = "test_default_rule"
    e = engine(n, mode=mode)
    e.set_solver(-1)
    e.set_pivoting(pivot)
    c = e.mode()[1]
    bad = run(e, [window(n)], who, f"default mode {mode} chunk {c}", pivot, chunk=c)
    e.close()
    report(who, bad, pivot)


@PIVOT
@pytest.mark.parametrize("mode", [1, 0], ids=["latency", "bandwidth"])
def test_default_rule_18_windows(mode, pivot):
    who = "test_default_rule"
    e = engine(64, windows=18, mode=mode)
    e.set_solver(-1)
    e.set_pivoting(pivot)
    c = e.mode()[1]
    bad = run(e, [window(64, seed=200 + k) for k in range(18)], who, f"default W=18 mode {mode} chunk {c}", pivot, chunk=c, fetch=(0, 7, 17))
    e.close()
    report(who, bad, pivot)


def _propagated_prior(w):
    """A prior the way the reference means it (test_BA_reg_with_a_propagated_prior_vs_oracle): the last Hessian block of the C2
    chain propagated along the window and sampled at its frames."""
    from conftest import load_golden
    from vinsat_amd import prior
    win, t, st0 = w
    g = load_golden("c2")
    dur = int(t[-1] - t[0])
    omega = np.random.default_rng(3).normal(0, 1e-3, (dur + 1, 3))
    ref0 = win.states_gt
    st_t, _v, Hs_t, _Hr = prior.propagate_dynamics_cov_init(ref0[0], ref0[0, 7:], g["last_hessian_19"][0], omega, 0, dur, 1)
    rows = (t - t[0]).astype(int)
    return st_t[rows], Hs_t[rows]


@PIVOT
@pytest.mark.parametrize("n", [25, 50])
def test_ba_reg(n, pivot):
    who = "test_ba_reg"
    w = window(n)
    e = engine(n)
    e.set_solver(2, -1)
    e.set_pivoting(pivot)
    bad = run(e, [w], who, "BA_reg chunk 2", pivot, chunk=2, prior=_propagated_prior(w))
    e.close()
    report(who, bad, pivot)


@PIVOT
def test_long_gap_window(pivot):
    who = "test_long_gap_window"
    gaps = np.random.default_rng(26).integers(1, 61, size=25)
    gaps[[7, 18]] = 700
    e = engine(26)
    e.set_solver(2, -1)
    e.set_pivoting(pivot)
    bad = run(e, [window(26, gaps=gaps)], who, "gaps 1..60 s, two of 700 s", pivot, chunk=2)
    e.close()
    report(who, bad, pivot)


# ---------------------------------------------------------------------------------------------------------------- comparison build
@pytest.mark.variants
@PIVOT
@pytest.mark.parametrize("what,n,c", [("packed", 47, 0), ("packed", 100, 0), ("cr-one-level", 47, 2), ("cr-one-level", 100, 2),
                                      ("resident-front", 100, 4), ("resident-front", 200, 8), ("resident", 100, 4), ("resident", 200, 8)])
def test_comparison_solvers(what, n, c, pivot):
    """The solvers of the comparison build that tests/test_gpu_variants.py reaches bit for bit, each against its own system:
    three windows per wavefront (k_solve_packed: five windows of equal pose count), one cyclic-reduction level in front
    (fusion bit 4) and the solve as one grid of waiting blocks (bits 5 / 6; the dispatch takes it from chunks of 4 and 24
    separators on, on a latency-mode handle whose chunk elimination forms its blocks)."""
    who = "test_comparison_solvers"
    if what == "packed":
        e = engine(n, windows=5)
        e.set_solver(-3)
        # windows that stay on the unpivoted kernels (47 poses: seed 300 does not, 100 poses: one of 400 .. 404 does not;
        # test_packed_walk_pivoted_fallback has the one that falls back)
        wins = [window(n, seed=(400 if n == 47 else 300) + k) for k in range(5)]
    else:
        sep = (n + c - 1) // c - 1
        if what.startswith("resident"):
            assert c >= 4 and 24 <= sep <= 256         # what launch_comparison_t asks before it launches k_solve_resident
        e = engine(n, mode=1)
        e.set_solver(c, -1)
        e.set_fusion({"cr-one-level": 9 + 16, "resident-front": 15 + 32, "resident": 15 + 64}[what])
        wins = [window(n)]
    e.set_pivoting(pivot)
    bad = run(e, wins, who, f"{what} chunk {c}", pivot, chunk=c)
    e.close()
    report(who, bad, pivot)


@pytest.mark.variants
def test_packed_walk_pivoted_fallback():
    """Five 47-pose windows, three per wavefront, unpivoted handle: the window of seed 300 fails the pivot check of call 14 and
    must be repeated by k_solve_packed<true> alone in its group while the others keep their unpivoted result.  Every window
    against its own system, by the bars of the pivoted kernels (which window ran where is the library's business)."""
    who = "test_packed_walk_pivoted_fallback"
    e = engine(47, windows=5)
    e.set_solver(-3)
    bad = run(e, [window(47, seed=300 + k) for k in range(5)], who, "packed with a fallback", True, falls_back=True)
    e.close()
    report(who, bad, True)
