"""Windows on the seams of the median select (vinsat_amd/csrc/vba_obs.hip ``k_obs_residual``, vba_select.hip, vba_select_body.h).  No GPU
needed (the library's host code is: build first).  Every window has 16 poses (``leaving``: 8) and at most 4097 rows, and is made once
per session.

The rows are drawn from one pool (``trial_cases.rich(16, 260)``: 4160 rows, states a tenth of the driver's perturbation off the truth)
and measured anew: ``uv = O.landmark_project(states, ...) + delta``, so the keys of a call at ``states`` are |delta| to within ~1e-13
(the device's projection rounds differently).  A group of rows that is to share the top 32 bits of its keys -- the bits KNOWN behind
digit 2; the compacted list is keyed on fewer, ``key >> 42``, and every other row lies below 2 or above 3.5 px, outside the group's
list under either reading -- has the offset 2.7 (9.3 in ``stale``) +- 1e-7: mixed low mantissa bits, so that neither the noise nor the jitter -- which makes the keys of the group differ, so
that a select that returns a neighbour is seen -- carries into the compared bits.  A group that is to tie bit
for bit -- also one call later, at other states -- is one row repeated (same landmark, pose and measurement) with confidence 0: its
keys count in the median and it does not pull the step.  Copies of one row measured +- 1e-7 apart share their projection at every
state: their keys differ, and differ by the same amounts one call later (``tied-bin``, ``long-ties``).

Fresh windows (``fresh(m, dist)``; the keys of the first call):
  spread              |delta| over 5 binades, either sign; m in KEY_COUNTS: 256 rows per block of ``k_obs_residual``, 1024 rows = 2048
                      keys per block of ``k_select_pass<.,.,8>``, 4096 rows = 8192 keys per block at 32 keys per thread
  wide                1e-6 .. 1e5 px: the median's exponent bin is short, many digit-0 bins are populated
  zeros               spread, and 40 % of the rows measured where they project (delta = +-0): tiny keys and exact zeros below the median
  prefix-1024-*       512 rows at +-2.7 in both components, the others below 2 and above 3.5 px, counted so that the wanted rank is
  prefix-1026-*       entry 0 / the middle / the last of the list (``-first``, ``-mid``, ``-last``); 513 rows for a list of 1026
                      (``prefix-1026-last`` needs 1026 rows: the last of 1026 entries is rank 1025)
  all-tied            every row at +-2.7: with m = m_max the list is as long as its capacity (``base + off < 2 * m_max`` on its edge);
                      m = 1025 (digits) and m = 512 (a list of exactly 1024 = its capacity, ranked by counting)
Carried windows (``carried(name)``; two landmark-only calls, the second selects among the keys the first one's trial left):
  tied-bin            600 rows: one row of pose 0 40 times +- 1e-7 without weight; 275 rows below 2 / above 3.5 px twice, measured off
                      in opposite directions (their poses stay put); 10 rows of pose 8 measured 6 px off, which fall under the group
                      when their pose follows them -- the second call wants entry 51 of the group's 80 different keys, 20 ranks
                      under the first call's median, where the warm bins begin
  dup-bin             the same with 40 exact copies: the median is one of equal keys and not the first of them
  long-bin            2100 rows, 80 % of them within 10 % of 2.7 px: the warm bin of the median is long at shift 51 (1040 rows come
                      twice, measured off in opposite directions: the step stays small and the band narrow)
  long-ties           2100 rows built the same way: 1100 copies, 450 pairs, 100 movers -- 1399 different keys of the group fill the last
                      sub-bin of the first digit of the bin under the first call's median, with keys of other rows earlier in the bin
  m4097               4097 rows, spread
  leaving             8 poses x 40 rows from the driver's initial guess: the median falls below half of the first call's
  rising              600 rows: 240 measured 30 px off in one direction, 360 without weight near 1 px -- the poses follow the weighted
                      rows and the median rises past the upper end of the range at shift 42
"""
from dataclasses import replace

import numpy as np

import dynamics_cases as D
import trial_cases as T
from oracle import ba_oracle as O

KEY_COUNTS = (1, 2, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097)
DISTS_1025 = ("spread", "wide", "zeros", "prefix-1024-first", "prefix-1024-mid", "prefix-1024-last", "prefix-1026-first", "prefix-1026-mid",
              "prefix-1026-last", "all-tied")
RAGGED_ROWS = (1025, 1, 256)
BATCH16_ROWS = (2, 255, 257, 1, 256, 64, 3, 130, 2, 257, 17, 255, 1, 100, 256, 31)
CARRIED = ("tied-bin", "long-bin", "long-ties", "m4097", "leaving", "rising", "dup-bin")
# fresh case -> (branch, list length, wanted rank inside the list); every other fresh case: ``count`` on a list of fewer than 9 keys
FRESH_BRANCH = {"prefix-1024-first[1025]": ("count", 1024, 0), "prefix-1024-mid[1025]": ("count", 1024, 512),
                "prefix-1024-last[1025]": ("count", 1024, 1023), "prefix-1026-first[1025]": ("digits", 1026, 0),
                "prefix-1026-mid[1025]": ("digits", 1026, 513), "prefix-1026-last[1026]": ("digits", 1026, 1025),
                "all-tied[1025]": ("digits", 2050, 1024), "all-tied[512]": ("count", 1024, 511), "stale-first[1025]": ("digits", 2050, 1024)}
SHORT_LIST = 9
DEFAULT_SWITCH_WINDOWS = 200                    # more than kLatWindowsCap = 192: a handle that chooses for itself takes the bandwidth set
IT, LAM = D.IT_INIT, D.LAM_INIT                 # the landmark-only call of the cases
OFFSET, STALE_OFFSET = 2.7, 9.3
JITTER = 1e-7                                   # 2.7 lies 1.9e-7 above the next value whose top 32 bits differ, 7.6e-7 below the one after
_CASES = {}


def pool():
    return T.rich(16, 260)


def _mags(rng, k, lo, hi):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), (k, 2))) * rng.choice([-1.0, 1.0], (k, 2))


def _banded(rng, group, nb, nx, na, offset=OFFSET, signed=True, jitter=True):
    """[group + nb + nx + na, 2] offsets: ``group`` rows at +-offset in both components, nb rows below 2 px, nx rows with one component
    below and one above, na rows above 3.5 px.  2 nb + nx keys lie below the group's."""
    g = np.full((group, 2), offset)
    if jitter:
        g = g + rng.uniform(-JITTER, JITTER, (group, 2))
    if signed:
        g = g * rng.choice([-1.0, 1.0], (group, 2))
    mix = np.concatenate([_mags(rng, nx, 0.3, 2.0)[:, :1], _mags(rng, nx, 3.5, 20.0)[:, :1]], -1)
    return np.concatenate([g, _mags(rng, nb, 0.3, 2.0), mix, _mags(rng, na, 3.5, 20.0)])


def _split(below):
    """(nb, nx) rows for ``below`` keys under the group."""
    return below // 2, below % 2


def _build(name, take, delta, conf=None, shuffle=None):
    p = pool()
    take, delta = np.asarray(take, dtype=np.int64), np.asarray(delta, dtype=np.float64)
    conf = p.conf[take].copy() if conf is None else np.asarray(conf, dtype=np.float64)
    if shuffle is not None:
        o = shuffle.permutation(take.size)
        take, delta, conf = take[o], delta[o], conf[o]
    xyz, ii = p.xyz[take].copy(), p.ii[take].copy()
    est = O.landmark_project(p.states, xyz, p.K, ii, jacobian=False)
    return replace(p, name=name, xyz=xyz, uv=est + delta, conf=conf, ii=ii)


def _delta(rng, m, dist):
    if dist == "spread":
        return np.exp2(rng.uniform(-2.0, 3.0, (m, 2))) * rng.choice([-1.0, 1.0], (m, 2))
    if dist == "wide":
        return 10.0 ** rng.uniform(-6.0, 5.0, (m, 2)) * rng.choice([-1.0, 1.0], (m, 2))
    if dist == "zeros":
        d = _delta(rng, m, "spread")
        z = rng.permutation(m)[:(2 * m) // 5]
        d[z] = 0.0 * rng.choice([-1.0, 1.0], (z.size, 2))
        return d
    if dist == "all-tied":
        return (OFFSET + rng.uniform(-JITTER, JITTER, (m, 2))) * rng.choice([-1.0, 1.0], (m, 2))
    if dist.startswith("prefix-"):
        _p, length, where = dist.split("-")
        group = int(length) // 2
        rank = (2 * m - 1) // 2
        below = rank - {"first": 0, "mid": group, "last": 2 * group - 1}[where]
        nb, nx = _split(below)
        na = m - group - nb - nx
        assert below >= 0 and na >= 0, (dist, m)
        return _banded(rng, group, nb, nx, na)
    raise ValueError(dist)


def fresh(m, dist="spread"):
    """The fresh window of ``m`` rows and distribution ``dist`` (a ``dynamics_cases.Case``; its states are the pool's)."""
    key = ("fresh", m, dist)
    if key not in _CASES:
        seed = 100 * m + sorted(DISTS_1025 + ("stale",)).index(dist)
        rng = np.random.default_rng(seed)
        take = rng.permutation(pool().m)[:m]
        off = _delta(rng, m, dist)
        _CASES[key] = _build(f"{dist}[{m}]", take, off, shuffle=rng)
    return _CASES[key]


def rows_1025(dist):
    return 1026 if dist == "prefix-1026-last" else 1025


def stale():
    """(first, second): 1025 rows all at +-9.3, then 256 spread rows for the same slot."""
    key = ("stale",)
    if key not in _CASES:
        rng = np.random.default_rng(77)
        take = rng.permutation(pool().m)[:1025]
        first = _build("stale-first[1025]", take, (STALE_OFFSET + rng.uniform(-JITTER, JITTER, (1025, 2))) * rng.choice([-1.0, 1.0], (1025, 2)))
        _CASES[key] = (first, fresh(256, "spread"))
    return _CASES[key]


def ragged():
    return [fresh(m, "spread") for m in RAGGED_ROWS]


def batch16():
    return [fresh(m, "spread") for m in BATCH16_ROWS]


def batch_over_the_switch():
    """200 windows (the 16 of ``batch16`` in turn)."""
    b = batch16()
    return [b[k % len(b)] for k in range(DEFAULT_SWITCH_WINDOWS)]


MOVER_BIAS = 6.0


def _repeated(rng, copies, pairs_below, pairs_above, movers, jitter=True):
    """A window around one row of pose 0 repeated ``copies`` times with confidence 0, measured +2.7 off in both components (+- 1e-7 each
    with ``jitter``: the copies share their projection at every state, so their keys differ and differ by the same amounts one call
    later).  The other rows come in pairs measured off in opposite directions -- below 2 px and above 3.5 px -- which cancel in the
    normal equations: their poses, pose 0 among them, stay where they are.  ``movers`` rows of pose 8 are all measured +6 px off: that
    pose follows them, and their 2 x movers keys fall from above the group to below it.  So the second call wants a key of the group
    2 x movers ranks under the first call's median, where the warm bins begin: a bin that ends with the group."""
    p = pool()
    own = [rng.permutation(np.nonzero(p.ii == k)[0]) for k in range(p.n)]
    rest = rng.permutation(np.concatenate([own[k][1:] if k == 0 else own[k] for k in range(p.n) if k != 8]))
    pairs = pairs_below + pairs_above
    half = np.concatenate([_mags(rng, pairs_below, 0.3, 2.0), _mags(rng, pairs_above, 3.5, 20.0)])
    g = np.full((copies, 2), OFFSET) + (rng.uniform(-JITTER, JITTER, (copies, 2)) if jitter else 0.0)
    take = np.concatenate([np.full(copies, own[0][0]), rest[:pairs], rest[:pairs], own[8][:movers]])
    off = np.concatenate([g, half, -half, MOVER_BIAS + rng.normal(0.0, 0.05, (movers, 2))])
    conf = p.conf[take].copy()
    conf[:copies] = 0.0
    return take, off, conf


def carried(name):
    key = ("carried", name)
    if key in _CASES:
        return _CASES[key]
    rng = np.random.default_rng(500 + CARRIED.index(name))
    if name == "tied-bin":
        # 600 rows, rank 599: 528 keys below, so the first call wants entry 71 of the group's 80 keys and the second entry 51
        c = _build(name, *_repeated(rng, 40, 132, 143, 10), shuffle=rng)
    elif name == "dup-bin":
        c = _build(name, *_repeated(rng, 40, 132, 143, 10, jitter=False), shuffle=rng)
    elif name == "long-ties":
        # 2100 rows, rank 2099: 700 keys below, entry 1399 of the group's 2200 keys, then entry 1199: 1399 keys of the group end the bin
        c = _build(name, *_repeated(rng, 1100, 175, 275, 100), shuffle=rng)
    elif name == "long-bin":
        # 1040 rows twice, the second time measured off the other way: the pairs cancel in the normal equations, so that the step --
        # which 20 single rows cause -- leaves the narrow band narrow
        pairs, single = 1040, 20
        k = (pairs * 4) // 5
        half = np.concatenate([_mags(rng, k, 0.9 * OFFSET, 1.1 * OFFSET), _mags(rng, (pairs - k) // 2, 0.3, 2.0),
                               _mags(rng, pairs - k - (pairs - k) // 2, 3.5, 20.0)])
        rows = rng.permutation(pool().m)[:pairs + single]
        take = np.concatenate([rows[:pairs], rows[:pairs], rows[pairs:]])
        c = _build(name, take, np.concatenate([half, -half, _mags(rng, single, 0.3, 2.0)]), shuffle=rng)
    elif name == "m4097":
        c = replace(fresh(4097, "spread"), name=name)
    elif name == "leaving":
        c = _leaving()
    elif name == "rising":
        m, heavy = 600, 240
        take = rng.permutation(pool().m)[:m]
        off = np.concatenate([np.full((heavy, 2), 30.0) + rng.normal(0.0, 0.5, (heavy, 2)), _mags(rng, m - heavy, 0.7, 1.4)])
        conf = pool().conf[take].copy()
        conf[heavy:] = 0.0
        c = _build(name, take, off, conf, shuffle=rng)
    else:
        raise ValueError(name)
    _CASES[key] = c
    return c


LEAVING_SEED = 3


def _leaving(seed=LEAVING_SEED):
    """8 poses x 40 rows at the driver's initial guess (tests/test_select_reference_host.py: the oracle's median more than halves)."""
    from vinsat_amd import od_pipe
    g, _fixed = D.gaps_for(8, "mixed", 7100 + seed)
    frames_t = np.concatenate([[D.T0], D.T0 + np.cumsum(g)]).astype(np.int64)
    win = od_pipe.prepare_window(*D.sequence(frames_t, 40, 7100 + seed))
    st = od_pipe.initial_guess(win, seed=seed)
    return D.Case("leaving", st, win.landmarks_xyz.copy(), win.landmarks_uv.copy(), win.confidences.copy(), win.ii.astype(np.int64),
                  win.intrinsics.copy(), win.cumrot_last.copy(), frames_t, win.states_gt.copy())


# ------------------------------------------------------------------------------------------------ the oracle's view
def sorted_order(ii):
    return np.argsort(np.asarray(ii, dtype=np.int64), kind="stable")


def device_order(keys, ii):
    """[m, 2] keys in input order -> the 2 m keys as the device holds them (rows sorted by pose, stable)."""
    return np.asarray(keys, dtype=np.float64)[sorted_order(ii)].reshape(-1)


def oracle_keys(c, states=None):
    st = c.states if states is None else states
    return np.abs(c.uv - O.landmark_project(st, c.xyz, c.K, c.ii, jacobian=False))


def oracle_call(c):
    """The oracle's landmark-only call on ``c``: (keys at its states [m, 2], median there, keys at the states it returns, trials)."""
    key = ("oracle", c.name, c.m)
    if key not in _CASES:
        out, _lam, _h, ntr = O.ba_iteration(IT, c.states, c.cumrot, c.uv, c.xyz, c.ii, c.t, c.K, c.conf, LAM, initialize=True)
        k0 = oracle_keys(c)
        _CASES[key] = (k0, float(np.sort(k0.reshape(-1))[(k0.size - 1) // 2]), oracle_keys(c, out), ntr)
    return _CASES[key]
