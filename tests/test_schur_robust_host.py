"""The restatement behind the tests of ``vba_schur_reweight`` (tests/schur_robust_reference.py), on the CPU without a device: it is
the reference's weighting (``oracle/ba_oracle.py:robust_weights``) bit for bit, its float64 rounding stays inside the cap the device
is held to, each bar of the GPU tests can fail, the planted window separates under the oracle, and the API exists.
"""
import os
import re

import numpy as np
import pytest

import schur_cases as C
import schur_robust_reference as RR
from oracle import ba_oracle as O


def _r12():
    d = RR.case("12")
    return d, RR.residuals(d, d["states0"], d["Xs"])


def test_restatement_is_the_oracles_weighting_bit_for_bit():
    d, r = _r12()
    assert r.shape == (577, 2)
    rng = np.random.default_rng(3)
    conf = np.where(rng.random(r.shape[0]) < 0.1, 0.0, rng.uniform(0.5, 1.0, r.shape[0]))      # the base weight plays conf
    for it in range(7):
        alpha = O.lm_schedule(it)[0]
        w, c, wmax = O.robust_weights(r, it, conf)
        got, gc, gmax = RR.weights_f64(r, alpha, conf)
        assert np.array_equal(got, w) and gc == c and gmax == wmax
        assert c == RR.lower_median(RR.keys_of(r))


def test_alpha_schedule_is_the_references():
    from vinsat_amd import schur
    for it in range(26):
        assert schur.alpha_schedule(it) == O.lm_schedule(it)[0]
    assert schur.alpha_schedule(0) == 2 and schur.alpha_schedule(5) == 1


def test_alpha_two_is_exactly_one():
    d, r = _r12()
    rho, c, wmax = RR.rho_f64(r, 2.0)
    assert np.all(rho == 1.0) and wmax == 1.0 / c ** 2
    assert np.all(RR.rho_ld(r, 2.0, c) == 1)


@pytest.mark.parametrize("name", ["12", "43", "129"])
def test_float64_restatement_stays_inside_the_cap(name):
    """The cap of the exact chain (32 ulp) is a condition on the device; the NumPy float64 chain must meet it itself."""
    d = RR.case(name)
    r = RR.residuals(d, d["states0"], d["Xs"])
    for alpha in RR.ALPHAS:
        rho, c, _ = RR.rho_f64(r, alpha)
        dev = RR.rel_dev(rho * d["w"], RR.rho_ld(r, alpha, c) * d["w"].astype(RR.LD))
        print(f"FIGURES schur robust host {name} alpha={alpha}: float64 against longdouble rho * base {dev:.3e} (cap {RR.ULP_CAP:.3e})")
        assert dev < RR.ULP_CAP


def test_a_median_of_the_upper_rank_misses_the_bit_bar():
    d, r = _r12()
    keys = RR.keys_of(r)
    assert keys.size % 2 == 0
    assert RR.lower_median(keys, keys.size // 2) != RR.lower_median(keys)


def test_a_maximum_taken_after_the_base_weights_misses_the_weight_bar():
    d, r = _r12()
    rng = np.random.default_rng(4)
    base = rng.uniform(0.2, 1.0, r.shape[0])
    base[int(np.argmax(RR.rho_f64(r, 1.0)[0]))] = 0.2            # the row of the largest raw weight has a small base weight
    rho, c, _ = RR.rho_f64(r, 1.0)
    good = rho * base
    q = rho * base
    wrong = q / q.max()
    assert RR.rel_dev(good, RR.rho_ld(r, 1.0, c) * base.astype(RR.LD)) < RR.ULP_CAP
    assert RR.rel_dev(wrong, RR.rho_ld(r, 1.0, c) * base.astype(RR.LD)) > 1e3 * RR.ULP_CAP


def test_keys_without_the_rows_of_weight_zero_miss_the_bit_bar():
    d, r = _r12()
    w = d["w"].copy()
    w[np.argsort(np.abs(r).max(-1))[: r.shape[0] // 10]] = 0.0          # the best-fitting tenth of the rows gets weight 0
    assert RR.lower_median(RR.keys_of(r[w > 0])) != RR.lower_median(RR.keys_of(r))


def test_planted_window_separates_under_the_oracle():
    """The condition of the end-to-end GPU test, confirmed with the oracle and the driver's own stopping rule."""
    d = RR.planted()
    st, X, rho, hist = RR.oracle_robust_solve(d, outer=8)
    worst, others = RR.planted_figures(d, rho)
    print(f"FIGURES schur robust host planted: largest rho of a planted row {worst:.4f}, median rho of the others {others:.4f}, "
          f"c_obs per round {[round(c, 3) for c, _ in hist]}")
    assert len(hist) == 8
    assert worst < RR.RHO_PLANTED_MAX and others > RR.RHO_OTHERS_MEDIAN_MIN


def test_select_constants_are_readable():
    k = RR.select_constants()
    assert k["kSelDigitBits"] * (64 // k["kSelDigitBits"]) == 64 and k["kSelThreads"] == 1 << k["kSelDigitBits"]
    assert k["kSelSmallMax"] >= k["kSelThreads"] * k["kSelKeysPerThread"]


def test_the_api_exists():
    with open(os.path.join(C.ROOT, "include", "vinsat_ba.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for proto in (r"int vba_schur_reweight\(vba_schur_handle h, double alpha, double\* c_obs, double\* w_max, int\* status\);",
                  r"int vba_schur_get_weights\(vba_schur_handle h, double\* w\s*, double\* base\s*\);",
                  r"int vba_schur_last_reweight_ms\(vba_schur_handle h, float\* ms\);",
                  r"int vba_schur_median\(int device, const double\* keys, int64_t count, double\* median\);"):
        assert re.search(proto, header), proto
    from vinsat_amd import schur
    for name in ("reweight", "weights", "last_reweight_ms"):
        assert callable(getattr(schur.SchurBA, name))
    assert callable(schur.median) and callable(schur.alpha_schedule)
    import inspect
    assert inspect.signature(schur.SchurBA.solve).parameters["robust"].default is None
