"""``vba_schur_reweight`` / ``SchurBA.reweight`` on the GPU (``include/vinsat_ba.h`` carries the contract).

Exact chains: ``c_obs`` is the lower median of the device's OWN keys bit for bit; the weights are held, from the device's own keys
and ``c_obs``, to the longdouble ``rho * base`` within 32 ulp (tests/schur_robust_reference.py: ``ULP_CAP``, a condition whose
float64 NumPy counterpart tests/test_schur_robust_host.py asserts); the keys to the longdouble restatement within four times the
float64 restatement's own deviation from it.  The promise: after a re-weighting the handle gives, bit for bit, what a fresh handle
gives that was built with ``weights()`` and the same state.  Every test needs the entry points and fails where they do not exist.

End to end (``solve(robust=dict(outer=8))`` on the planted window of tests/schur_robust_reference.py): the oracle with the same
driver gives 0.0372 for the largest ``rho`` of a planted row and 0.7135 for the median ``rho`` of the others
(tests/test_schur_robust_host.py asserts both limits on it); the condition for the device is ``< 0.1`` and ``> 0.5``.
"""
from ctypes import byref, c_double, c_int, c_void_p

import numpy as np
import pytest

import schur_robust_reference as RR

pytestmark = pytest.mark.gpu
NAMES = ("12", "43", "129")
LAM = 1e-3
REL_OUTPUTS = ("leverage", "wtest", "lm_leverage", "lm_wtest", "lm_stats", "pose_stats")
EINVAL, ESTATE = 1, 4


def _open(d, w=None, state=None, uv=None):
    from vinsat_amd.schur import SchurBA
    e = SchurBA(d["states0"], d["X0"], d["uv"] if uv is None else uv, d["w"] if w is None else w, d["pose_of_row"], d["landmark_of_row"],
                d["intrinsics"], sigma_prior=d["sigma"])
    e.set_state(*(state or (d["states0"], d["Xs"])))
    return e


def _sparse_weights(d):
    """The case's weights, 10 % of them zero and the others spread (seeded)."""
    rng = np.random.default_rng(31)
    w = rng.uniform(0.3, 1.0, d["w"].size)
    w[rng.permutation(w.size)[: w.size // 10]] = 0.0
    return w


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def _median_of_own_keys(e, res):
    keys = e.reweight_keys().reshape(-1)
    assert keys.size == 2 * e.m and not np.signbit(keys).any()
    want = np.sort(keys)[(keys.size - 1) // 2]
    assert _bits_equal(res["c_obs"], want), (res["c_obs"], want)
    return keys.reshape(-1, 2)


def _crit90(rel, w):
    t = np.concatenate([rel["wtest"][w > 0.0], rel["lm_wtest"]])
    return float(np.percentile(t[np.isfinite(t)], 90)) / float(np.sqrt(rel["fit"]["s0sq"]))


def _totals(e):
    tot = (c_int * 3)()
    e._check(e.lib.vba_schur_rejected(e.h, None, None, tot))
    return tuple(tot)


def _same_rel(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in REL_OUTPUTS) and a["info"] == b["info"] and \
        np.array_equal(np.array(list(a["fit"].values())), np.array(list(b["fit"].values())), equal_nan=True)


def _same_cov(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in ((a["pose"], b["pose"]), (a["landmark"], b["landmark"]), (a["pairs"][2], b["pairs"][2])))


def _same_iterate(a, b, lam=LAM):
    ra, rb = a.iterate(lam), b.iterate(lam)
    sa, sb = a.get_state(), b.get_state()
    return ra == rb and all(_bits_equal(x, y) for x, y in zip(a.last_step() + sa, b.last_step() + sb)) and a.last_info() == b.last_info()


@pytest.mark.parametrize("name", NAMES)
def test_median_keys_and_weights_exact_chains(name):
    d = RR.case(name)
    st, X = d["states0"], d["Xs"]
    e = _open(d)
    order = e.order
    k64 = RR.keys_of(RR.residuals(d, st, X)[order])
    kld = RR.keys_of(RR.residuals(d, st, X, RR.LD)[order])
    floor = float(np.abs(k64.astype(RR.LD) - kld).max() / kld.max())
    for alpha in RR.ALPHAS:
        res = e.reweight(alpha)
        assert res["status"] == 0 and res["c_obs"] > 0.0 and res["w_max"] > 0.0
        keys = _median_of_own_keys(e, res)
        kdev = float(np.abs(keys.reshape(-1).astype(RR.LD) - kld).max() / kld.max())
        want = RR.rho_ld(keys, alpha, res["c_obs"]) * d["w"][order].astype(RR.LD)
        wdev = RR.rel_dev(e.weights()[order], want)
        print(f"FIGURES schur robust {name} alpha={alpha}: keys against longdouble {kdev:.3e} (float64 restatement {floor:.3e}, bar {4 * floor:.3e}); "
              f"rho * base against longdouble from the device's keys {wdev:.3e} (cap {RR.ULP_CAP:.3e}); c_obs {res['c_obs']!r} w_max {res['w_max']!r} "
              f"{e.last_reweight_ms():.3f} ms")
        assert kdev <= 4 * floor
        assert wdev < RR.ULP_CAP
        assert _bits_equal(e.weights(base=True), d["w"])
        if alpha == 2.0:
            assert _bits_equal(e.weights(), d["w"]) and res["w_max"] == 1.0 / (res["c_obs"] * res["c_obs"])
    assert e.last_reweight_ms() > 0.0
    e.close()


@pytest.mark.parametrize("name", NAMES)
def test_rows_of_weight_zero_count_in_the_median(name):
    d = RR.case(name)
    w = _sparse_weights(d)
    e, plain = _open(d, w=w), _open(d)
    for alpha in (1.2, 1.0):
        res, ref = e.reweight(alpha), plain.reweight(alpha)
        keys = _median_of_own_keys(e, res)
        assert res["c_obs"] == ref["c_obs"] and res["w_max"] == ref["w_max"]        # the base weights enter neither
        got = e.weights()
        assert np.all(got[w == 0.0] == 0.0)
        assert RR.rel_dev(got[e.order], RR.rho_ld(keys, alpha, res["c_obs"]) * w[e.order].astype(RR.LD)) < RR.ULP_CAP
    # ... and after a snoop that rejected rows
    e.reweight(2.0)
    rel = e.reliability(LAM)
    got = e.snoop(LAM, _crit90(rel, w), True, 6, 3)
    assert got["rows"] > 0
    for alpha in (1.2, 1.0):
        res, ref = e.reweight(alpha), plain.reweight(alpha)
        _median_of_own_keys(e, res)
        assert res["c_obs"] == ref["c_obs"] and res["w_max"] == ref["w_max"]
    e.close()
    plain.close()


@pytest.mark.parametrize("name", NAMES)
def test_handle_behaves_as_a_fresh_one_with_those_weights(name):
    d = RR.case(name)
    e = _open(d, w=_sparse_weights(d))
    before = e.iterate(LAM)
    seen = (e.get_state(), e.last_info(), e.last_ms(), e.last_step(), e.cholesky_factor() if name == "12" else None)
    res = e.reweight(1.2)
    assert res["status"] == 0
    # state, last_info, last_ms, debug_fetch(0 / 1) read as before the call
    now = (e.get_state(), e.last_info(), e.last_ms(), e.last_step(), e.cholesky_factor() if name == "12" else None)
    assert all(_bits_equal(x, y) for x, y in zip(seen[0] + seen[3], now[0] + now[3])) and seen[1:3] == now[1:3]
    assert name != "12" or _bits_equal(seen[4], now[4])
    w = e.weights()
    assert not _bits_equal(w, e.weights(base=True))
    f = _open(d, w=w, state=e.get_state())
    assert _same_cov(e.covariance(LAM, pairs=True), f.covariance(LAM, pairs=True))
    rel_e, rel_f = e.reliability(LAM), f.reliability(LAM)
    assert _same_rel(rel_e, rel_f)
    assert _same_iterate(e, f)
    crit = _crit90(rel_e, w)
    se, sf = e.snoop(LAM, crit, True, 6, 3), f.snoop(LAM, crit, True, 6, 3)
    assert se == sf and se["rows"] > 0
    assert all(np.array_equal(x, y) for x, y in zip(e.rejected(), f.rejected()))
    assert _bits_equal(e.weights(), f.weights())
    assert _same_iterate(e, f)
    assert before[0] > 0.0
    e.close()
    f.close()


@pytest.mark.parametrize("name", NAMES)
def test_alpha_two_puts_the_uploaded_weights_back(name):
    d = RR.case(name)
    w = _sparse_weights(d)
    e, never = _open(d, w=w), _open(d, w=w)
    for alpha in (1.0, 1.6):
        assert e.reweight(alpha)["status"] == 0
        assert not _bits_equal(e.weights(), w)
    assert e.reweight(2.0)["status"] == 0
    assert _bits_equal(e.weights(), w) and _bits_equal(e.weights(base=True), w) and _bits_equal(e.weights(), e.weights(base=True))
    assert _bits_equal(never.weights(), w) and _bits_equal(never.weights(base=True), w)
    assert _same_iterate(e, never) and _same_iterate(e, never, 1e-6)
    e.close()
    never.close()


def _upload(e, d, w):
    """``vba_schur_upload`` of the handle's own structure again, with the weights ``w`` (caller's row order)."""
    s, o = e.structure, e.order
    p = lambda a: a.ctypes.data_as(c_void_p)
    u, v = np.ascontiguousarray(d["uv"][o, 0]), np.ascontiguousarray(d["uv"][o, 1])
    ws, K, X0 = np.ascontiguousarray(w[o]), np.ascontiguousarray(d["intrinsics"], dtype=np.float64), np.ascontiguousarray(d["X0"])
    e._check(e.lib.vba_schur_upload(e.h, p(s["lm_ptr"]), p(s["row_pose"]), p(s["row_lm"]), p(u), p(v), p(ws), p(s["pose_ptr"]), p(s["pose_rows"]),
                                    p(s["blk_i"]), p(s["blk_j"]), p(s["blk_ptr"]), p(s["pair_k"]), p(s["pair_k2"]), p(K), p(X0), float(d["sigma"])))


@pytest.mark.parametrize("name", NAMES)
def test_snoop_then_reweight_then_restore(name):
    from vinsat_amd import _lib
    d = RR.case(name)
    w = _sparse_weights(d)
    e, plain = _open(d, w=w), _open(d, w=w)
    assert _bits_equal(e.weights(base=True), w)
    rel = e.reliability(LAM)
    got = e.snoop(LAM, _crit90(rel, w), True, 6, 3)
    assert got["rows"] > 0
    rows, lms = e.rejected()
    totals = _totals(e)
    assert _bits_equal(e.weights(), np.where(rows, 0.0, w)) and _bits_equal(e.weights(base=True), w)     # rejected rows report their saved value
    res, ref = e.reweight(1.2), plain.reweight(1.2)
    assert res == ref and res["status"] == 0
    now = e.weights()
    assert np.all(now[rows] == 0.0) and not np.signbit(now[rows]).any()
    assert _bits_equal(now[~rows], plain.weights()[~rows])
    assert all(np.array_equal(x, y) for x, y in zip(e.rejected(), (rows, lms))) and _totals(e) == totals
    e.restore_rejected()
    assert _bits_equal(e.weights(), plain.weights())            # rho * base on every row: the handle that never snooped
    assert not e.rejected()[0].any() and _totals(e) == (0, 0, 0)
    assert _same_rel(e.reliability(LAM), plain.reliability(LAM))
    assert e.reweight(2.0)["status"] == 0
    assert _bits_equal(e.weights(), w)
    # a new upload clears the feature state: its weights are the base of the next re-weighting
    e.reweight(1.0)
    w2 = np.where(w > 0.0, 0.5 * w + 0.1, 0.0)
    _upload(e, d, w2)
    assert _bits_equal(e.weights(), w2) and _bits_equal(e.weights(base=True), w2)
    with pytest.raises(_lib.VbaError):
        e.reweight_keys()
    fresh = _open(d, w=w2)
    assert e.reweight(1.0) == fresh.reweight(1.0)
    assert _bits_equal(e.weights(), fresh.weights()) and _bits_equal(e.weights(base=True), w2)
    for x in (e, plain, fresh):
        x.close()


def test_a_state_that_fits_exactly_changes_nothing():
    """Every residual exactly 0 on the device: with ``uv = 0`` the keys of a re-weighting are ``|est|`` of the device itself, and
    ``sign(est)`` is the oracle's (no projection of this window is near 0)."""
    d = RR.case("12")
    w = _sparse_weights(d)
    probe = _open(d, uv=np.zeros_like(d["uv"]))
    assert probe.reweight(2.0)["status"] == 0
    est_dev = np.empty_like(d["uv"])
    est_dev[probe.order] = probe.reweight_keys()
    probe.close()
    est = d["uv"] - RR.residuals(d, d["states0"], d["Xs"])
    assert np.abs(est).min() > 1.0 and np.abs(est_dev - np.abs(est)).max() < 1e-6
    e = _open(d, w=w, uv=np.sign(est) * est_dev)
    res = e.reweight(1.2)
    assert not e.reweight_keys().any()
    assert res["status"] == 1 and res["c_obs"] == 0.0 and np.isnan(res["w_max"])
    assert _bits_equal(e.weights(), w) and _bits_equal(e.weights(base=True), w)
    e.close()


def test_a_nan_residual_changes_nothing():
    d = RR.case("12")
    w = _sparse_weights(d)
    uv = d["uv"].copy()
    uv[5, 0] = np.nan
    e = _open(d, w=w, uv=uv)
    res = e.reweight(1.2)                                       # c_obs is finite, the largest raw weight is not (numpy's max)
    assert res["status"] == 1 and np.isfinite(res["c_obs"]) and np.isnan(res["w_max"])
    assert _bits_equal(e.weights(), w)
    uv[:] = np.nan
    f = _open(d, w=w, uv=uv)
    res = f.reweight(1.2)
    assert res["status"] == 1 and np.isnan(res["c_obs"]) and np.isnan(res["w_max"]) and _bits_equal(f.weights(), w)
    e.close()
    f.close()


def test_errors():
    from vinsat_amd import _lib
    from vinsat_amd.schur import build_structure
    d = RR.case("12")
    e = _open(d)
    c, wm, st = c_double(), c_double(), c_int()
    for alpha in (0.99, 2.01, float("nan")):
        assert e.lib.vba_schur_reweight(e.h, alpha, byref(c), byref(wm), byref(st)) == EINVAL
        with pytest.raises(_lib.VbaError):
            e.reweight(alpha)
    assert e.lib.vba_schur_reweight(e.h, 1.5, None, byref(wm), byref(st)) == EINVAL
    assert _bits_equal(e.weights(), d["w"])
    # before a state is set (and before the upload): a handle of the same sizes by the C entry points alone
    lib, h = e.lib, c_void_p()
    s = e.structure
    assert lib.vba_schur_create(0, e.n, e.m, e.L, int(s["blk_i"].size), int(s["pair_k"].size), byref(h)) == 0
    assert lib.vba_schur_reweight(h, 1.5, byref(c), byref(wm), byref(st)) == ESTATE
    raw = type(e).__new__(type(e))
    raw.lib, raw.h, raw.structure, raw.order, raw.n, raw.m, raw.L = lib, h, s, e.order, e.n, e.m, e.L
    _upload(raw, d, d["w"])
    assert lib.vba_schur_reweight(h, 1.5, byref(c), byref(wm), byref(st)) == ESTATE
    out = np.empty(2 * e.m)
    assert lib.vba_schur_debug_fetch(h, 2, out.ctypes.data_as(_lib.PD), out.size) == ESTATE
    raw.set_state(d["states0"], d["Xs"])
    assert lib.vba_schur_reweight(h, 1.5, byref(c), byref(wm), byref(st)) == 0 and st.value == 0
    assert lib.vba_schur_debug_fetch(h, 2, out.ctypes.data_as(_lib.PD), out.size - 1) == EINVAL
    assert (c.value, wm.value, 0) == tuple(e.reweight(1.5).values())
    raw.close()
    e.close()


@pytest.mark.parametrize("name", NAMES)
def test_two_handles_give_equal_bits(name):
    d = RR.case(name)
    w = _sparse_weights(d)
    a, b = _open(d, w=w), _open(d, w=w)
    for alpha in (1.6, 1.0):
        ra, rb, again = a.reweight(alpha), b.reweight(alpha), a.reweight(alpha)
        assert ra == rb == again
        assert _bits_equal(a.weights(), b.weights()) and _bits_equal(a.reweight_keys(), b.reweight_keys())
    a.close()
    b.close()


def test_robust_solve_downweights_the_planted_rows():
    from vinsat_amd import schur
    d = RR.planted()
    e = _open(d)
    hist = e.solve(robust=dict(outer=8))
    rounds = [h[1] for h in hist if h[0] == "reweight"]
    assert len(rounds) == 8 and all(r["status"] == 0 for r in rounds)
    assert rounds[0]["w_max"] == 1.0 / rounds[0]["c_obs"] ** 2 and schur.alpha_schedule(0) == 2      # the first call is plain least squares
    rho = e.weights() / e.weights(base=True)
    worst, others = RR.planted_figures(d, rho)
    trials = sum(1 for h in hist if h[0] != "reweight")
    print(f"FIGURES schur robust planted: largest rho of a planted row {worst:.4f} (oracle 0.0372), median rho of the others {others:.4f} "
          f"(oracle 0.7135), {trials} LM trials, c_obs per round {[round(r['c_obs'], 3) for r in rounds]}")
    assert worst < RR.RHO_PLANTED_MAX and others > RR.RHO_OTHERS_MEDIAN_MIN
    # robust=None is the plain loop: two handles, the same bits
    a, b = _open(d), _open(d)
    assert a.solve(max_iters=3) == b.solve(max_iters=3, robust=None)
    for x in (e, a, b):
        x.close()
