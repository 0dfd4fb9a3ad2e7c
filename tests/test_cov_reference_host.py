"""The judge of tests/cov_reference.py on the cases of tests/cov_cases.py (no GPU, no library): the longdouble reference against
itself, the levels of the four fp64 references, and the proof that the bars of tests/test_gpu_covariance_paths.py can fail --
planted faults must exceed them by a wide margin.

Systems: the bands of the NumPy oracle (cov_cases.oracle_bands, call 14) for every single-window case and every window of the two
batches, undamped and damped, at two stages, each held to every condition below on its own:
  start   at the case's start states (the initial guess, lamda 1e-4) -- where the conditions on the cases are set;
  query   at the states two oracle calls (9 and 10) leave from there -- the systems the device query of
          tests/test_gpu_covariance_paths.py meets; less well conditioned than the start states, so the harder set.

Measured (400 rows per pose, 60 s between frames, 46 windows of 2 .. 120 poses):
  longdouble   recurrence against the dense inverse (n <= 10) 4.0e-14 in the scaled metric; |A^ Sigma - I| / (|A^| |Sigma|) 2.6e-14
               for the dense inverse and 9.6e-13 for the recurrence, whose residual carries the cancellation of A^ Sigma = I.
  fp64, largest scaled figure of any case per reference and over all groups:
    start      LU inverse 5.6e-11, Cholesky 3.7e-11, block recurrence 9.2e-11 (both n = 2 of a batch), partitioned 6.3e-11
               (chunks of 3, n = 7); largest of any case and group 9.2e-11 (diag pos-pos), velocity-velocity 4.2e-11
    query      LU inverse 4.0e-10 (n = 25), Cholesky 1.7e-10, block recurrence 1.3e-10 (n = 120), partitioned 5.4e-10 (chunks of
               12, n = 25); largest of any case and group 5.4e-10 (diag pos-pos), velocity-velocity 4.5e-10
  no case raises ZERO_PIVOT or INDEFINITE at either stage; smallest eigenvalue at the start states +7.8 .. +37 against 4e10.
  faults       smallest (largest figure of the faulted result) / (16 x largest fp64 figure of any case and group of the stage),
               required >= 100:              start                                  query
               (a) Sigma_SS from the neighbour   4.2e8 (s = 2, n = 9)               6.7e7 (s = 2, n = 9)
               (b) correction left out           6.8e8 (s = 60, n = 120)            1.2e8 (s = 8, n = 16)
               (c) one-pose last chunk at D^-1   6.8e8 (s = 60, n = 61)             1.2e8 (s = 60, n = 61)
               (d) super block transposed        1.9e8 (s = 60, n = 61)             3.8e7 (s = 8, n = 9)
               (e) 1e-6 in one vel-vel block     678                                117
Fault (e) also passes block_rel_err at 1e-8 (asserted): the gap the scaled metric closes.
"""
import numpy as np
import pytest

import cov_cases as K
import cov_oracle as C
import cov_reference as R

M = 16                      # tests/test_gpu_covariance_paths.py
MARGIN = 100.0              # a planted fault must exceed M times the largest fp64 figure of any case by this factor
STAGES = ("start", "query")  # the case's start states; the states the device query meets (calls 9 and 10 later)


@pytest.fixture(scope="module")
def systems():
    """{(n, seed, stage): (bands, lam32, {damped: longdouble selected inverse})} of every window of the cases at both stages
    (STAGES), computed once."""
    wins = {(n, n) for _, n in K.all_single_cases()}
    for s, n_max in K.BATCHES:
        wins |= {(n, 500 + 10 * s + k) for k, n in enumerate(K.batch(s, n_max))}
    out = {}
    for n, seed in sorted(wins):
        for stage in STAGES:
            bands, lam = K.oracle_bands(K.window(n, seed), stage == "query")
            lam32 = float(np.float32(lam))
            out[(n, seed, stage)] = (bands, lam32, {d: R.selected_inverse_ld(bands, lam32 if d else 0.0) for d in (False, True)})
    return out


def _cases():
    """[(s, n, seed)]: the single-window cases and the windows of the batches (s = 0: the sequential walk, judged with one chunk)."""
    out = [(s, n, n) for s, n in K.all_single_cases()]
    for s, n_max in K.BATCHES:
        out += [(s, n, 500 + 10 * s + k) for k, n in enumerate(K.batch(s, n_max))]
        out += [(0, n, 500 + 10 * s + k) for k, n in enumerate(K.batch(s, n_max))]
    return out


@pytest.fixture(scope="module")
def figures(systems):
    """({stage: {key: largest fp64 figure of any case}}, {(s, n, seed, stage, damped): Levels})."""
    top, lvs = {st: dict.fromkeys(R.KEYS, 0.0) for st in STAGES}, {}
    for s, n, seed in _cases():
        for stage in STAGES:
            bands, lam32, refs = systems[(n, seed, stage)]
            for d in (False, True):
                lv = R.levels(bands, lam32 if d else 0.0, s if s else n, ref=refs[d])
                lvs[(s, n, seed, stage, d)] = lv
                for k in R.KEYS:
                    top[stage][k] = max(top[stage][k], lv.cpu[k])
    return top, lvs


def test_the_reference_checks_itself(systems):
    """Recurrence against the dense inverse, both longdouble (n <= 10), in the scaled componentwise metric, and the residual
    |A^ Sigma - I| of both against |A^| |Sigma|.  Bars from the number format: the fp64 references of these systems reach 5e-10 with
    a unit roundoff of 2^-53, so the same algorithms in longdouble (2^-64) are expected near 2^-11 of that, 3e-13; the bar is
    1e-11, a fiftieth of the fp64 level.  The residual of the recurrence carries the cancellation of A^ Sigma = I on top: 1e-10;
    a wrong block gives a figure of order 1 in either."""
    worst_e = worst_r = worst_rs = 0.0
    for (n, seed, stage), (bands, lam32, refs) in systems.items():
        for d in (False, True):
            lam = lam32 if d else 0.0
            rd, rs = refs[d]
            rel = R.identity_residual(bands, lam, rd, rs)
            worst_rs = max(worst_rs, rel)
            assert rel < 1e-10, (n, seed, stage, d, rel)
            assert not rs[n - 1].any() and np.array_equal(rd, rd.transpose(0, 2, 1))
            if n > 10:
                continue
            A, inv = R.dense_inverse_ld(bands, lam)
            res = np.abs(A @ inv - np.eye(9 * n)) / (np.abs(A) @ np.abs(inv))
            worst_r = max(worst_r, float(res.max()))
            assert float(res.max()) < 1e-10, (n, seed, d)
            dd, ds = C.blocks_of(inv, n)
            e = R.scaled_err(rd, rs, dd, ds).worst
            worst_e = max(worst_e, e[0])
            assert e[0] < 1e-11, (n, seed, d, e)
    print(f"\nlongdouble: recurrence against dense inverse {worst_e:.2e}; residual / (|A||Sigma|): dense {worst_r:.2e}, recurrence {worst_rs:.2e}")


def test_conditions_on_the_cases(systems, figures):
    """No case raises ZERO_PIVOT or INDEFINITE in the fp64 recurrence; the largest fp64 figures per group are printed (the module
    docstring records them); test_planted_faults_exceed_the_bars holds the faults against them."""
    top, lvs = figures
    for (n, seed, stage), (bands, lam32, _) in systems.items():
        for lam in (0.0, lam32):
            assert R.recurrence_flags(bands, lam) == 0, (n, seed, stage, lam)
    for stage in STAGES:
        by_ref = {}
        for key, lv in lvs.items():
            for name, v in lv.by_ref.items():
                if key[3] == stage and v > by_ref.get(name, (0.0, None))[0]:
                    by_ref[name] = (v, key)
        print(f"\n{stage}: largest fp64 figure per reference:", {k: f"{v:.2e} at {at}" for k, (v, at) in by_ref.items()})
        print(f"{stage}: largest fp64 figure per group:", {k: f"{v:.2e}" for k, v in top[stage].items()})


def _fault_cases():
    return [(("a", 1), 2, 9), (("a", 3), 2, 9), (("a", 0), 5, 16), (("a", 0), 12, 25),
            (("b", "first"), 5, 11), (("b", "last"), 5, 11), (("b", "first"), 2, 5), (("b", "last"), 8, 16), (("b", "last"), 60, 120),
            (("c",), 2, 3), (("c",), 5, 11), (("c",), 8, 33), (("c",), 60, 61),
            (("d", 0), 2, 2), (("d", 3), 5, 9), (("d", 4), 5, 9), (("d", 7), 8, 9), (("d", 59), 60, 61),
            (("e", 0), 2, 2), (("e", 5), 5, 11), (("e", 4), 5, 11), (("e", 60), 60, 120)]


@pytest.mark.parametrize("damped", [False, True], ids=["undamped", "damped"])
@pytest.mark.parametrize("stage", STAGES)
def test_planted_faults_exceed_the_bars(systems, figures, stage, damped):
    """Every fault of cov_reference.partitioned_fp64 exceeds M times the largest fp64 figure of ANY case of its stage (any group)
    by the factor MARGIN in at least one group pair, and is turned away by ``judge`` with the case's own bars.  Fault (e) also
    passes tests/cov_oracle.py's block_rel_err at its 1e-8 bar: the gap this metric closes."""
    top, lvs = figures
    level = max(max(top[stage].values()), R.EPS)
    least, short = {}, []
    for fault, s, n in _fault_cases():
        bands, lam32, refs = systems[(n, n, stage)]
        lam = lam32 if damped else 0.0
        lv = lvs[(s, n, n, stage, damped)]
        good = R.partitioned_fp64(bands, lam, s)
        assert R.judge(*good, lv, M).ok
        got = R.partitioned_fp64(bands, lam, s, fault=fault)
        v = R.judge(*got, lv, M)
        assert not v.ok, (fault, s, n)
        val, key, _pose = v.err.worst
        margin = val / (M * level)
        least[fault[0]] = min(least.get(fault[0], (np.inf,)), (margin, key, s, n))
        if not margin >= MARGIN:
            short.append((fault, s, n, f"{margin:.3g}", key))
        if fault[0] == "e":
            ref = (refs[damped][0].astype(np.float64), refs[damped][1].astype(np.float64))
            assert key == "diag vel-vel" and _pose == fault[1]
            assert C.block_rel_err(got[0], ref[0]) < 1e-8 and C.block_rel_err(got[1][:n - 1], ref[1][:n - 1]) < 1e-8
    print(f"\n{stage}: largest fp64 figure of any case {level:.3g}; smallest margin per fault (figure / (16 x that), group, s, n):",
          {k: (f"{m:.3g}", key, s, n) for k, (m, key, s, n) in least.items()})
    assert not short, short
