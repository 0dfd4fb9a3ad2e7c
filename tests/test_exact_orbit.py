"""tests/exact_orbit.py: the long-double chain of one-second RK4 steps that the long-gap GPU tests measure against.

Measured on the states of tests/golden/gap.npz before call 25 (25 poses, each walked for s steps): the fp64 oracle
(O.propagate_orbit) lies from the exact chain, worst edge, position / velocity max-rel and Phi position / velocity columns:
    s = 1:     6.3e-17 / 5.6e-17,  1.1e-16 / 3.1e-16
    s = 65:    5.5e-16 / 9.1e-16,  1.2e-15 / 8.6e-16
    s = 935:   4.3e-15 / 4.9e-15,  3.8e-15 / 2.9e-15
    s = 3000:  2.3e-14 / 3.3e-14,  2.7e-14 / 2.8e-14
-- rounding of fp64 that grows along the chain (the oracle's own walk is thus no anchor below ~1e-14 at 3000 s)."""
import numpy as np
import pytest

import exact_orbit as X
from conftest import load_golden
from oracle import ba_oracle as O

# (steps, bar on every component of the fp64 oracle against the exact chain): twice the drift measured above
DRIFT = [(1, 7e-16), (65, 2.5e-15), (935, 1e-14), (3000, 7e-14)]


def _gap_states():
    st = load_golden("gap")["states_out_24"][0]
    return np.concatenate([st[:, :3], st[:, 7:]], -1)


@pytest.mark.parametrize("s,bar", DRIFT, ids=[str(s) for s, _ in DRIFT])
def test_fp64_oracle_is_within_its_rounding_drift_of_the_exact_chain(s, bar):
    x = _gap_states()
    steps = np.full(x.shape[0], s)
    xh, Phi = O.propagate_orbit(x, steps)
    xe, Pe = X.propagate(x, steps)
    errs = X.edge_errors(xh, Phi, xe, Pe)
    for name, e in zip(("pos", "vel", "Phi pos cols", "Phi vel cols"), errs):
        assert e.max() <= bar, (name, e.max())
    # ... and the exact chain is not the fp64 one: at hundreds of steps the two differ somewhere
    if s >= 65:
        assert max(e.max() for e in errs) > 1e-17
    # the state alone (no tangents) is the same chain
    assert np.array_equal(X.propagate(x[:3], steps[:3], stm=False), xe[:3])


@pytest.mark.parametrize("s", [65, 935])
def test_exact_sensitivity_agrees_with_central_differences_of_the_exact_chain(s):
    """Phi of the long-double chain against (x_hat(x + d e_k) - x_hat(x - d e_k)) / 2d of the same chain: d = 1e-3 km for the
    position columns, 1e-6 km/s for the velocity columns (truncation ~ (d / r)^2 relative, rounding ~ eps_ld |x| / d)."""
    x = _gap_states()[[0, 12, 24]]
    steps = np.full(x.shape[0], s)
    _, Pe = X.propagate(x, steps)
    for k in range(6):
        d = X.LD(1e-3 if k < 3 else 1e-6)
        xp = x.astype(X.LD)
        xm = x.astype(X.LD)
        xp[:, k] += d
        xm[:, k] -= d
        col = (X.propagate(xp, steps, stm=False) - X.propagate(xm, steps, stm=False)) / (2 * d)
        err = np.abs(col - Pe[:, :, k]).max(1) / np.abs(Pe[:, :, k]).max(1)
        assert float(err.max()) < 1e-9, (k, float(err.max()))


def _radial_states(rng, n):
    """Start states falling (nearly) straight at the Earth's centre: 100 .. 1e5 km, 0.5 .. 12 km/s, a third exactly radial."""
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = 10 ** rng.uniform(2, 5, n)
    v = rng.uniform(0.5, 12, n)
    tang = rng.normal(size=(n, 3))
    tang -= (tang * d).sum(1, keepdims=True) * d
    tang *= (rng.uniform(0, 1e-3, n) * (rng.random(n) < 0.67))[:, None]
    return np.concatenate([d * r[:, None], (-d + tang) * v[:, None]], 1)


def _diverged_states(seed):
    """The oracle's states before the last call of the randomised schedule (the states the GPU diverged at)."""
    import random_windows
    win, xyz, uv, ii, conf, t, st0 = random_windows.make(seed, long_gaps=True)
    st, lam = st0.copy(), 1e-4
    for it, init in random_windows.SCHEDULE[:-1]:
        st, lam, _, _ = O.ba_iteration(it, st, win.cumrot_last, uv, xyz, ii, t, win.intrinsics, conf, lam, initialize=init)
    return st, O.step_counts(t)


def test_no_finite_state_found_whose_coarse_chain_alone_goes_non_finite():
    """vba_long.hip leaves the parareal iteration on a non-finite defect; a serial fallback would be owed to an edge whose
    coarse chain or linearised sweep goes non-finite while the serial walk stays finite (exact_orbit.coarse_chain).  Near-radial
    start states and the diverged states of seeds 315 / 318 (|c| / |x| of 1e2 .. 1e4 there: the coarse chain is far off) --
    none is such an edge."""
    rng = np.random.default_rng(7)
    for s in (65, 1038, 6000):
        ok, serial_ok, _ = X.coarse_chain(_radial_states(rng, 100), s)
        assert not (~ok & serial_ok).any(), s
    for seed in (315, 318):
        st, steps = _diverged_states(seed)
        x = np.concatenate([st[:, :3], st[:, 7:]], -1)
        far = 0.0
        for i in np.nonzero(steps[:-1] > 64)[0]:
            ok, serial_ok, cx = X.coarse_chain(x[i], steps[i])
            assert ok[0] and serial_ok[0], (seed, i)
            far = max(far, float(cx[0]))
        assert far > 1e2, (seed, far)         # (the coarse chain IS thrown far off at these states)
