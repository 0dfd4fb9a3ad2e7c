"""Windows and references of the layer-by-layer tests of the sharded stage kernels (tests/test_gpu_sharded_stages.py; the conditions on
the cases and the planted faults: tests/test_sharded_stage_cases_host.py).  NumPy only; every window is made once per session.

Windows (``dynamics_cases.Case``; rows in shuffled order, cut by ``vinsat_amd.dist.shard_bounds`` into contiguous slices):
  slices()            17 poses, 91 rows: 1, 16, 17 and 33 rows on poses 0 .. 3, none on pose 9, two on every other pose (cut like
                      ``query_windows._Small``).  Rows 12 .. 35 are rows of pose 3, so that at R = 8 ranks 1 and 2 lie inside one pose;
                      every other boundary falls inside a pose as well (a pose with rows on both sides); 91 is no multiple of 2, 3 or 8
  head(R + 1)         its first R + 1 rows: slices of 2, 1, 1, ... rows
  rejecting(conf)     slices() with confidences of 2.2 (the oracle's landmark-only call from lamda = 1e-4 rejects four trials and accepts
                      the fifth) or 3 (it rejects all nine): ``stage3(None, ...)`` runs
  chain()             608 poses (27 n = 16416 > 64 x 256: a second trip of the grid-stride loops of k_shard_pack / k_shard_reduce), two
                      rows per pose, every 50th pose without rows; R = 3
  select_case(name)   16 poses, keys planted with ``select_cases``' banded deltas around 2.7 px so that the median is a key of the band
                      with two different neighbours; R = 8.  One per branch of the select over gathered keys:
                        count            4096 rows, band of 512 keys <= 1024 = 2 m_local
                        digits           4160 rows, band of 1032 keys <= 1040 = 2 m_local
                        overflow-short   512 rows, band of 200 keys > 128 = 2 m_local
                        overflow-long    1024 rows, band of 1040 keys > 256 = 2 m_local
                        padded           515 rows: ranks 3 .. 7 hold 64 rows in slots of 65, so the gathered buffer holds +inf keys
                        all-tied         ``select_cases.fresh(512, "all-tied")``: 1024 keys in the list, 128 fit (overflow-short)

References: what a layer's output must be, from the outputs of the layer in front (``reduce_expected``, ``decide_expected``,
``sum_pred_model``) or from the rows in extended precision (``check_partial``, ``trial_figure``).  ``faults`` plant the mistakes the
host test shows to be caught."""
from dataclasses import replace

import numpy as np

import accumulate_reference as A
import dynamics_cases as D
import select_cases as SC
import select_reference as S
import trial_cases as T
import trial_reference as TR

LD = np.longdouble
U = 2.0 ** -53
IT_INIT, IT_FULL = 0, 12
CALLS = {"landmark": (IT_INIT, True, D.LAM_INIT), "full": (IT_FULL, False, D.LAM)}
SLICE_RANKS = (1, 2, 3, 8)
SELECT_RANKS = 8
CHAIN_N, CHAIN_RANKS = 608, 3
PACK_TRIP = 64 * 256                            # entries one trip of k_shard_pack / k_shard_reduce covers
SELECT = {"count": (4096, 256), "digits": (4160, 516), "overflow-short": (512, 100), "overflow-long": (1024, 520), "padded": (515, 20)}
SELECT_BRANCH = {"count": "count", "digits": "digits", "overflow-short": "overflow-short", "overflow-long": "overflow-long",
                 "padded": "count", "all-tied": "overflow-short"}
_CASES = {}


def bounds(m, ranks):
    from vinsat_amd.dist import shard_bounds
    return shard_bounds(m, ranks)


def rank_rows(c, ranks, r):
    b = bounds(c.m, ranks)
    return slice(int(b[r]), int(b[r + 1]))


def take_rows(c, rows, name=None):
    return replace(c, name=name or c.name, xyz=c.xyz[rows], uv=c.uv[rows], conf=c.conf[rows], ii=c.ii[rows])


# ------------------------------------------------------------------------------------------------ windows
SLICE_ROWS = {0: 1, 1: 16, 2: 17, 3: 33, 9: 0}


def slices():
    if "slices" not in _CASES:
        base = T.rich(17, 40)
        rng = np.random.default_rng(1717)
        keep = np.concatenate([np.nonzero(base.ii == i)[0][:SLICE_ROWS.get(i, 2)] for i in range(17)])
        p3 = keep[base.ii[keep] == 3][:24]
        rest = rng.permutation(np.setdiff1d(keep, p3))
        _CASES["slices"] = take_rows(base, np.concatenate([rest[:12], p3, rest[12:]]), "slices[91]")
    return _CASES["slices"]


def head(m):
    c = slices()
    return take_rows(c, slice(0, m), f"head[{m}]")


REJECT_CALL = (IT_INIT, True, 1e-4)               # landmark-only from the driver's first damping
REJECT_TRIALS = {2.2: 5, 3.0: 9}                 # confidence -> trials of the oracle (tests/test_sharded_stage_cases_host.py)


def rejecting(conf=2.2):
    """slices() with every confidence at ``conf``; the weighted trial residual grows with it while the initial one does not.  2.2: the
    oracle rejects four trials and accepts the fifth; 3 (as in tests/golden/rej.npz): it rejects all nine the damping allows."""
    c = slices()
    return replace(c, name=f"rejecting-{conf:g}[91]", conf=np.full_like(c.conf, conf))


def chain():
    if "chain" not in _CASES:
        base = T.rich(CHAIN_N, 2)
        rng = np.random.default_rng(608)
        keep = rng.permutation(np.nonzero(base.ii % 50 != 7)[0])
        _CASES["chain"] = take_rows(base, keep, f"chain[{CHAIN_N}]")
    return _CASES["chain"]


def select_case(name):
    if name == "all-tied":
        return SC.fresh(512, "all-tied")
    key = ("select", name)
    if key not in _CASES:
        m, group = SELECT[name]
        rng = np.random.default_rng(4200 + sorted(SELECT).index(name))
        takes = rng.permutation(SC.pool().m)[:m]
        _CASES[key] = SC._build(f"{name}[{m}]", takes, SC._delta(rng, m, f"prefix-{2 * group}-mid"), shuffle=rng)
    return _CASES[key]


def slice_properties(c, ranks):
    """What the slices of ``c`` over ``ranks`` ranks look like: dict with ``sizes``, ``padded`` (ranks whose slot is longer than their
    slice), ``split_poses`` (poses with rows on more than one rank), ``inside_one_pose`` (ranks of more than one row, all of one
    pose), ``single_row`` (ranks of one row), ``boundaries_inside_a_pose`` (boundaries with rows of one pose on both sides)."""
    b = bounds(c.m, ranks)
    sizes = np.diff(b)
    m_pad = -(-c.m // ranks)
    owner = np.repeat(np.arange(ranks), sizes)
    split = [i for i in range(c.n) if np.unique(owner[c.ii == i]).size > 1]
    inside = [r for r in range(ranks) if sizes[r] > 1 and np.unique(c.ii[b[r]:b[r + 1]]).size == 1]
    cut = [r for r in range(1, ranks) if np.intersect1d(c.ii[:b[r]], c.ii[b[r]:]).size > 0]
    return dict(sizes=sizes.tolist(), padded=[r for r in range(ranks) if sizes[r] < m_pad], split_poses=split, inside_one_pose=inside,
                single_row=[r for r in range(ranks) if sizes[r] == 1], boundaries_inside_a_pose=cut)


def gathered(keys, ii, m, ranks):
    """The gathered buffer of stage 2 from the [m, 2] keys in input order: every rank's keys in ITS pose-sorted order, padded with +inf."""
    b = bounds(m, ranks)
    m_pad = -(-m // ranks)
    out = np.full((ranks, 2 * m_pad), np.inf)
    for r in range(ranks):
        lo, hi = int(b[r]), int(b[r + 1])
        out[r, :2 * (hi - lo)] = SC.device_order(keys[lo:hi], ii[lo:hi])
    return out.reshape(-1)


# ------------------------------------------------------------------------------------------------ layer 3: the partial of a rank
def sym6(a, b):
    a, b = min(a, b), max(a, b)
    return a * 6 - (a * (a - 1)) // 2 + (b - a)


_SYM = np.array([[sym6(a, b) for b in range(6)] for a in range(6)])


def unpack_partial(part, n):
    """(H [n, 6, 6], b [n, 6], wmax, sum |r|) of a partial of 27 n + 2 doubles: 21 packed upper-triangle entries per pose, then 6."""
    part = np.asarray(part, dtype=np.float64)
    return part[:21 * n].reshape(n, 21)[:, _SYM], part[21 * n:27 * n].reshape(n, 6), float(part[27 * n]), float(part[27 * n + 1])


def pack_partial(H, b, wmax, sum_abs, faults=()):
    """The partial as ``k_shard_pack`` writes it.  ``second_trip_missing``: the entries behind the first 64 x 256 are not written (0)."""
    n = H.shape[0]
    iu = np.triu_indices(6)
    out = np.concatenate([H[:, iu[0], iu[1]].reshape(-1), np.asarray(b).reshape(-1), [wmax, sum_abs]]).astype(np.float64)
    if "second_trip_missing" in faults:
        out[PACK_TRIP:27 * n] = 0.0
    return out


def raw_weights(r, conf, c, it):
    """(w_raw conf [m], w_raw [m]) in longdouble: what the accumulation sums with before anything is divided by the largest raw weight
    (``k_obs_accumulate``: wc = robust_weight_raw * conf; the division is ``vba_debug_fetch``'s and the assembly's)."""
    one = np.ones(np.asarray(conf).shape[0])
    return A.weights_ld(r, conf, c, 1.0, it), A.weights_ld(r, one, c, 1.0, it)


def check_partial(c, rows, part, est, Jg, c_obs, it, nblk, where, wmax_slot=True, sum_slot=True):
    """A rank's partial against the extended-precision sums of its rows ``c[rows]`` (``est`` [m_r, 2], ``Jg`` [m_r, 2, 6] as the judged
    side reports them, ``c_obs`` the GLOBAL median): ([] or what is wrong, the figures in units of 2^-53 with their bars).
    ``wmax_slot`` / ``sum_slot`` False: that slot is not in use (carried keys: tests/test_gpu_sharded_carried.py) and is not judged."""
    sub = take_rows(c, rows)
    lv = A.oracle_levels(c.states, sub.xyz, c.K, sub.uv, sub.ii, sub.conf, it, c.n)
    H, b, wmax, sum_abs = unpack_partial(part, c.n)
    r = sub.uv - np.asarray(est, dtype=np.float64)
    wc, wraw = raw_weights(r, sub.conf, c_obs, it)
    a = A.layer_a(H, b, est, wc, Jg, sub.uv, sub.ii, c.n)
    v = A.judge(lv, a)
    bad = [f"{where}: {f}" for f in v.failures]
    empty = np.bincount(sub.ii, minlength=c.n) == 0
    if empty.any() and not (np.all(H[empty] == 0.0) and np.all(b[empty] == 0.0)):
        bad.append(f"{where}: a pose without rows on this rank does not hold exact zeros")
    figs = {k: (v.units[k], v.bars[k]) for k in v.units}
    if wmax_slot:
        wref = wraw.max()
        fw = float(abs(LD(wmax) - wref) / wref) / U
        if not fw <= lv.K("w"):
            bad.append(f"{where}: wmax slot {wmax!r}, the largest raw weight of the rank's rows is {float(wref)!r}: {fw:.3g} > K = {lv.K('w'):.3g} (x 2^-53)")
        figs["wmax"] = (fw, lv.K("w"))
    if sum_slot:
        keys = np.abs(r)
        ref = S.exact_sum(keys)
        bound = S.sum_bound(sub.m, nblk)
        fs = float(abs(LD(sum_abs) - ref) / ref) / U if ref > 0 else float(sum_abs != 0.0)
        if not abs(LD(sum_abs) - ref) <= bound * ref:
            bad.append(f"{where}: sum |r| slot {sum_abs!r}, the keys sum to {float(ref)!r}: {fs:.3g} > {bound / U:.0f} (x 2^-53)")
        figs["sum_abs"] = (fs, bound / U)
    return bad, figs


def oracle_partial(c, rows, c_obs, it, faults=()):
    """The fp64 NumPy oracle in the place of a rank: (partial, est, Jg) of the rows ``c[rows]`` at the median ``c_obs``."""
    from oracle import ba_oracle as O
    sub = take_rows(c, rows)
    est, Jg = O.landmark_project(c.states, sub.xyz, c.K, sub.ii)
    r = sub.uv - est
    alpha = A.lm_alpha(it)
    with np.errstate(divide="ignore", invalid="ignore"):
        per = (((r / c_obs) ** 2) / abs(alpha - 2) + 1) ** (alpha / 2 - 1) / (c_obs ** 2)
    wraw = per.mean(-1)
    H, b = O.accumulate(Jg, wraw * sub.conf, r, sub.ii, c.n)
    return pack_partial(H, b, wraw.max(), np.abs(r).sum(), faults), est, Jg


# ------------------------------------------------------------------------------------------------ layer 4: the rank-ordered reduction
def reduce_expected(parts, n, faults=()):
    """(Hraw [21 n], braw [6 n], wmax, sum |r|) as ``k_shard_reduce`` leaves them from the ranks' partials: plain fp64 additions from 0.0
    in rank order, the largest of the wmax slots.  ``reverse_rank_order``: the planted fault."""
    parts = [np.asarray(p, dtype=np.float64) for p in parts]
    if "reverse_rank_order" in faults:
        parts = parts[::-1]
    s = np.zeros(27 * n + 2)
    for p in parts:
        s = s + p
    return s[:21 * n], s[21 * n:27 * n], max(0.0, max(float(p[27 * n]) for p in parts)), float(s[27 * n + 1])


def fetched_expected(parts, n, faults=()):
    """``debug("H")`` [n, 6, 6] and ``debug("b")`` [n, 6] behind the reduction: every entry of the rank-ordered sum divided once by the
    largest wmax slot (``vba_debug_fetch``: ``tmp[sym6(a, b)] / wmax``, ``out[k] /= wmax``)."""
    Hraw, braw, wmax, _s = reduce_expected(parts, n, faults)
    return (Hraw / wmax).reshape(n, 21)[:, _SYM], (braw / wmax).reshape(n, 6)


# ------------------------------------------------------------------------------------------------ layer 5: the two trial sums, the decision
def _wave_sum(v):
    """``wave_sum``: the xor butterfly over 64 lanes, offsets 32, 16, 8, 4, 2, 1; every lane ends with the same value."""
    v = np.asarray(v, dtype=np.float64).copy()
    idx = np.arange(64)
    for s in (32, 16, 8, 4, 2, 1):
        v = v + v[idx ^ s]
    return float(v[0])


def _block_sum(v256):
    t = 0.0
    for w in range(4):
        t = t + _wave_sum(v256[64 * w:64 * w + 64])
    return t


def sum_pred_model(r_pred, sigma):
    """sqrt(sigma) sum |r_pred| in the device's order from the fetched ``r_pred`` [n - 1, 7] of a window without long edges:
    ``dynamics_block`` (8 lanes per pose: lane 0 adds its six |r_orbit| in sequence, lane 6 holds |f|; ``block_sum<256>`` per 32 poses),
    then ``decide_load`` / ``decide_finish`` (thread t adds the blocks t, t + 256, ...; wave sums; ((w0 + w1) + w2) + w3)."""
    rp = np.abs(np.asarray(r_pred, dtype=np.float64))
    n = rp.shape[0] + 1
    lanes = np.zeros(-(-n * 8 // 256) * 256)
    for i in range(n - 1):
        s = rp[i, 0]
        for k in range(1, 6):
            s = s + rp[i, k]
        lanes[8 * i], lanes[8 * i + 6] = s, rp[i, 6]
    per_thread = np.zeros(256)
    for b in range(lanes.size // 256):
        per_thread[b % 256] = per_thread[b % 256] + _block_sum(lanes[256 * b:256 * b + 256])
    w = [_wave_sum(per_thread[64 * k:64 * k + 64]) for k in range(4)]
    return (((w[0] + w[1]) + w[2]) + w[3]) * float(np.sqrt(np.float64(sigma)))


def decide_expected(parts, trials, n, m_total, initialize, sum_pred):
    """(init_residual, trial_residual) of ``decide_finish``'s sharded branch from the ranks' partials and trial sums, fp64 in its order."""
    denom = 2.0 * float(m_total) + (6.0 if initialize else 7.0) * float(n - 1) + 0.0
    so = reduce_expected(parts, n)[3]
    sh = float(trials[0][1])
    for t in trials:
        sh = sh + float(t[0])
    return (so + (0.0 if initialize else sum_pred) + 0.0) / denom, (sh + 0.0) / denom


def trial_figure(t0, uv, est, weight, ii):
    """(figure, bar) in units of 2^-53 of a rank's observation trial sum against the extended-precision sum of ``trial_reference.row_terms``
    of its rows.  The bar, as for a slot sum of tests/test_gpu_trial_paths.py: max(16, 4 x the figure of fp64 NumPy summing the same
    terms tile by tile of 256 rows and the tiles in sequence)."""
    wt, _raw = TR.row_terms(uv, est, weight, ii)
    ref = wt.sum()
    f64 = wt.astype(np.float64)
    own = 0.0
    for t in range(-(-f64.size // TR.TILE)):
        own = own + float(f64[t * TR.TILE:t * TR.TILE + TR.TILE].sum())
    if ref == 0:
        return float(t0 != 0.0), 16.0
    return float(abs(LD(t0) - ref) / ref) / U, max(16.0, 4.0 * float(abs(LD(own) - ref) / ref) / U)
