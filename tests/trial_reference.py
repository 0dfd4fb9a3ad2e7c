"""Judging what the trial kernel (``k_trial``, vinsat_amd/csrc/vba_trial.hip) leaves behind, in extended precision and in exact integer
terms (NumPy only, no GPU needed): the block sums of the accept test slot by slot, the trial mean formed from them, and the carried
keys with their histogram and bin buckets.

Sums.  A slot of ``part_trial`` / ``part_next`` is judged against the longdouble sum of the terms the kernel puts there, evaluated at
the trial STATES and WEIGHTS the judged side itself reports -- the step's and the retraction's errors do not loosen a sum's bar:

  observation slot t   rows [256 t, 256 t + 256) of the pose-sorted order: sum |du w| + |dv w| (``part_trial``) and sum |du| + |dv|
                       (``part_next``), du = fl(uv - est): the one fp64 subtraction both the kernel and the oracle make; the measure
                       is the error over the sum of these (non-negative) terms;
  pose-chain slot b    edges and poses of block b: sqrt(sigma) (sum |D (x_hat_i - x_i+1)| + |f_i|) per edge -- D = diag(1, 1, 1,
                       kVelCoeff ...), the orbit part left out for a long edge, |f_i| over kQuatCoeff under BA_reg as the reference
                       writes it -- and sum |r_prior_i| per pose under BA_reg.  Plain geometry: 256 edges and poses per slot.  16-lane
                       geometry (``FUSED`` 1 / 2 / 3): 15 edges per slot, pose j in slot min(j // 15, nblk_dyn - 1) -- the 16th pose
                       of a block is the next block's first unless there is no next block;
  long-edge slot k     sqrt(sigma) sum |D (x_hat - x_next)| of the k-th long edge, behind the pose-chain slots.
                       The orbit terms are differences of coordinates of ~7000 km: their measure is the component's scale of
                       tests/dynamics_reference.py (``factor_layer``: |x_i| + the increments + |x_i+1|), summed over the slot.
  every other slot     exactly 0.

Keys, histogram, buckets: bit patterns and counts, no tolerance.  ``warm_bin`` / ``warm_range_start`` restate vba_device.h, ``exp_digit``
the digit 0 of the exact select.

A figure passes at K x 2^-53, K = max(16, 4 x the figure of the fp64 NumPy oracle on the same case and quantity): ``oracle_levels``
measures the oracle (its own trial states, its own weights, fp64 sums in slot order).  No bar comes from a device run."""
import numpy as np

import dynamics_reference as R
import exact_orbit as X
from oracle import ba_oracle as O

LD = np.longdouble
U = R.U
TILE = 256
EDGES16 = 15                    # kEdgesPerBlock16
SEL_BINS = 2048
MARGIN = 0.99                   # the oracle's first trial must come in below this share of the initial residual


# ------------------------------------------------------------------------------------------------ device constants
def f64_bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def warm_range_start(c_bits, shift):
    """``warm_range_start`` of vba_device.h: the lower end of the 2046 warm bins for median bits ``c_bits`` (2^64 - 1: no range)."""
    c_bits = int(c_bits)
    binades = 2046 >> (52 - shift)
    down = (binades + 1) // 2
    e = c_bits >> 52
    if e <= down or e >= 0x7FE:
        return (1 << 64) - 1
    return c_bits - (down << 52)


def warm_bin(key_bits, lo, shift):
    """``warm_bin`` of vba_device.h for an array of key bit patterns: 0 below the range, 1 .. 2046 inside, 2047 above."""
    k = np.asarray(key_bits, dtype=np.uint64)
    lo = np.uint64(lo)
    below = k < lo
    d = (np.where(below, lo, k) - lo) >> np.uint64(shift)
    return np.where(below, 0, np.where(d < 2046, d + np.uint64(1), 2047)).astype(np.int64)


def exp_digit(key_bits):
    """Digit 0 of the exact select: the 10 bits (bits >> 53) & 1023."""
    return ((np.asarray(key_bits, dtype=np.uint64) >> np.uint64(53)) & np.uint64(1023)).astype(np.int64)


def sorted_order(ii):
    """Sorted position -> input row of the upload's counting sort (stable by pose)."""
    return np.argsort(np.asarray(ii, dtype=np.int64), kind="stable")


# ------------------------------------------------------------------------------------------------ geometry
def geometry(n_max, m_max, lanes16):
    """(observation slots, pose-chain slots) of ``part_trial`` on a handle of that size."""
    nblk_obs = -(-int(m_max) // TILE)
    nblk_dyn = (int(n_max) - 1 + EDGES16 - 1) // EDGES16 if lanes16 else -(-int(n_max) // TILE)
    return nblk_obs, nblk_dyn


def edge_slot(i, lanes16):
    return i // (EDGES16 if lanes16 else TILE)


def pose_slot(j, nblk_dyn, lanes16):
    return min(j // EDGES16, nblk_dyn - 1) if lanes16 else j // TILE


# ------------------------------------------------------------------------------------------------ terms
def row_terms(uv, est, weight, ii):
    """(weighted [m], raw [m]) terms of the rows in pose-sorted order, longdouble: |du w| + |dv w| and |du| + |dv|."""
    r = np.abs(R._ld(np.asarray(uv, dtype=np.float64) - np.asarray(est, dtype=np.float64)))
    order = sorted_order(ii)
    raw = r.sum(-1)[order]
    return (r * R._ld(weight)[:, None]).sum(-1)[order], raw


def chain_terms(states, time_idx, cumrot, sigma, initialize, hop=False, prior=None):
    """Per edge / pose of the pose chain at ``states`` (longdouble): dict with
      orbit, orbit_den [n - 1]   sqrt(sigma) sum |D (x_hat - x_next)| and the component scale behind it;
      att [n - 1]                sqrt(sigma) |f| (over kQuatCoeff under BA_reg);
      prior, prior_den [n]       sum |r_prior| and the sum of the absolute terms behind it (zeros without BA_reg);
      long [n - 1] bool          edges of more than 64 steps (never with the hop integrator).
    A landmark-only call has no pose-chain terms: zeros."""
    st = np.asarray(states, dtype=np.float64)
    n = st.shape[0]
    z = np.zeros(n - 1, dtype=LD)
    out = dict(orbit=z, orbit_den=z.copy(), att=z.copy(), prior=np.zeros(n, dtype=LD), prior_den=np.zeros(n, dtype=LD),
               long=np.zeros(n - 1, dtype=bool))
    if initialize:
        return out
    sq = np.sqrt(LD(sigma))
    x, xh, _Phi = R.orbit_ld(st, time_idx, hop)
    steps = O.step_counts(time_idx)[:-1]
    D = R._ld(R.D6)
    out["orbit"] = sq * (np.abs(xh - x[1:]) * D).sum(-1)
    inc = R._ld(steps)[:, None] * (np.abs(X._deriv(x[:-1])) + np.abs(X._deriv(xh))) / 2
    out["orbit_den"] = sq * ((np.abs(x[:-1]) + inc + np.abs(x[1:])) * D).sum(-1)
    f = np.abs(R.attitude_ld(st, cumrot).f)
    out["att"] = sq * (f / R.KQ if prior is not None else f)
    out["long"] = (steps > R.LONG_GAP) & (not hop)
    if prior is not None:
        out["prior"] = np.abs(R.prior_ld(st, prior)[0]).sum(-1)
        out["prior_den"] = R.prior_ld(st, prior, absolute=True)[0].sum(-1)
    return out


def slot_sums(uv, est, weight, ii, ch, n_max, m_max, lanes16, nblk_long=0, faults=()):
    """The reference of every slot: dict of (value, den) pairs of longdouble arrays
      obs, raw [nblk_obs]     ``part_trial`` / ``part_next`` of the observation tiles;
      dyn [nblk_dyn]          the pose-chain slots;
      long [nblk_long]        the long edges' slots in pose order.
    ``ch``: ``chain_terms`` at the same states.  ``faults``: planted mistakes for the host test (names below)."""
    nblk_obs, nblk_dyn = geometry(n_max, m_max, lanes16)
    wt, raw = row_terms(uv, est, weight, ii)
    m = wt.size
    obs, rw = np.zeros(nblk_obs, dtype=LD), np.zeros(nblk_obs, dtype=LD)
    for t in range(-(-m // TILE)):
        lo, hi = t * TILE, min(m, t * TILE + TILE)
        if "boundary_row_twice" in faults and t > 0:
            lo -= 1                                     # the last row of the tile in front counted again
        obs[t], rw[t] = wt[lo:hi].sum(), raw[lo:hi].sum()
    if "tile_one_slot_late" in faults and nblk_obs > 1:
        obs, rw = np.roll(obs, 1), np.roll(rw, 1)
    n = ch["prior"].size
    dyn, dden = np.zeros(nblk_dyn, dtype=LD), np.zeros(nblk_dyn, dtype=LD)
    for i in range(n - 1):
        if "drop_16th_edge" in faults and lanes16 and i == EDGES16 - 1:
            continue                                    # the edge into the 16th pose of block 0
        b = edge_slot(i, lanes16)
        o, od = (0, 0) if ch["long"][i] else (ch["orbit"][i], ch["orbit_den"][i])
        dyn[b] += o + ch["att"][i]
        dden[b] += od + ch["att"][i]
    for j in range(n):
        if "drop_last_prior" in faults and j == n - 1:
            continue
        b = pose_slot(j, nblk_dyn, lanes16)
        dyn[b] += ch["prior"][j]
        dden[b] += ch["prior_den"][j]
    lidx = np.nonzero(ch["long"])[0]
    lg, lden = np.zeros(nblk_long, dtype=LD), np.zeros(nblk_long, dtype=LD)
    lg[:lidx.size], lden[:lidx.size] = ch["orbit"][lidx], ch["orbit_den"][lidx]
    return dict(obs=(obs, obs.copy()), raw=(rw, rw.copy()), dyn=(dyn, dden), long=(lg, lden))


def trial_mean(ref, n, m, initialize, reg):
    """(mean, den) of the accept test's trial residual from the slot references: the denominator of vba_decide.h (2 m + 6 or 7 per
    edge, and per pose under BA_reg), BA_reg's constant of 100 per pose in a full-phase call."""
    per = 6 if initialize else 7
    denom = LD(2 * m + per * (n - 1) + (per * n if reg else 0))
    c = LD(100 * n) if (reg and not initialize) else LD(0)
    tot = ref["obs"][0].sum() + ref["dyn"][0].sum() + ref["long"][0].sum() + c
    den = ref["obs"][1].sum() + ref["dyn"][1].sum() + ref["long"][1].sum() + c
    return tot / denom, den / denom


def slot_figures(ref, part_trial, part_next, nblk_long, exact):
    """Figures of a fetched ``part_trial`` [trial_stride] (``part_next`` [nblk_obs] or None) against ``ref``: dict name -> array per
    slot.  What lies behind the window's slots must be exactly 0: noted in ``exact``, as a slot without terms that is not."""
    pt = np.asarray(part_trial, dtype=np.float64)
    no, nd = ref["obs"][0].size, ref["dyn"][0].size
    figs = {"part_obs": R._ratio(np.abs(R._ld(pt[:no]) - ref["obs"][0]), ref["obs"][1], "part_trial observation slot", exact),
            "part_dyn": R._ratio(np.abs(R._ld(pt[no:no + nd]) - ref["dyn"][0]), ref["dyn"][1], "part_trial pose-chain slot", exact)}
    if nblk_long:
        figs["part_long"] = R._ratio(np.abs(R._ld(pt[no + nd:no + nd + nblk_long]) - ref["long"][0]), ref["long"][1],
                                     "part_trial long-edge slot", exact)
    rest = pt[no + nd + nblk_long:]
    if np.any(rest != 0):
        exact.append(f"part_trial: slot {no + nd + nblk_long + int(np.argmax(rest != 0))} behind the window's blocks is not 0")
    if part_next is not None:
        figs["part_next"] = R._ratio(np.abs(R._ld(part_next) - ref["raw"][0]), ref["raw"][1], "part_next slot", exact)
    if not np.isfinite(pt).all():
        exact.append("non-finite block sum")
    return figs


def retract_figure(states, dpose, states_new, exact):
    return R._ratio(np.abs(R._ld(states_new) - R.retract_ld(states, dpose)), R.retract_ld(states, dpose, absolute=True), "retract", exact)


def hessian_figure(last_hessian, H_last, lam32, exact):
    """``last_hessian`` of a landmark-only call against H / w_max of the last pose (as fetched) on the 6x6, zeros elsewhere, plus the
    damping on the diagonal."""
    ref = np.zeros((9, 9), dtype=LD)
    ref[:6, :6] = R._ld(H_last)
    ref = ref + LD(lam32) * np.eye(9, dtype=LD)
    return R._ratio(np.abs(R._ld(last_hessian) - ref), np.abs(ref), "last_hessian", exact)[None]


# ------------------------------------------------------------------------------------------------ keys, histogram, buckets
def expected_keys(uv, est):
    """|uv - est| as the kernel forms it: one fp64 subtraction, then the sign dropped."""
    return np.abs(np.asarray(uv, dtype=np.float64) - np.asarray(est, dtype=np.float64))


def key_bins(keys, kind, warm_lo, shift):
    bits = f64_bits(np.asarray(keys, dtype=np.float64).reshape(-1))
    return warm_bin(bits, warm_lo, shift) if kind == 2 else exp_digit(bits)


def check_keys(keys, uv, est):
    want = expected_keys(uv, est)
    diff = f64_bits(keys).reshape(-1) != f64_bits(want).reshape(-1)
    if diff.any():
        k = int(np.argmax(diff))
        return [f"carried key {k % 2} of row {k // 2}: {np.asarray(keys).reshape(-1)[k]!r} where |uv - est| is {want.reshape(-1)[k]!r}"
                f" ({int(diff.sum())} keys differ)"]
    return []


def check_hist(keys, kind, warm_lo, shift, hist, c_obs=None, sel_rank=None):
    """The histogram against the count per bin of the restated bin function over ``keys`` (any shape); its total is their number."""
    bad = []
    keys = np.asarray(keys, dtype=np.float64).reshape(-1)
    hist = np.asarray(hist).astype(np.int64)
    nb = SEL_BINS if kind == 2 else 1024
    if hist.size != nb:
        return [f"histogram of {hist.size} bins, kind {kind} has {nb}"]
    if kind == 2 and c_obs is not None and warm_lo != warm_range_start(int(f64_bits([c_obs])[0]), shift):
        bad.append(f"warm_lo {warm_lo:#x} is not warm_range_start of the call's median {c_obs!r} at shift {shift}")
    if kind == 1 and sel_rank is not None and sel_rank != (keys.size - 1) // 2:
        bad.append(f"sel_rank[0] {sel_rank} is not the lower median's rank {(keys.size - 1) // 2}")
    want = np.bincount(key_bins(keys, kind, warm_lo, shift), minlength=nb)
    if int(hist.sum()) != keys.size:
        bad.append(f"histogram total {int(hist.sum())}, {keys.size} keys")
    d = np.nonzero(hist != want)[0]
    if d.size:
        bad.append(f"histogram bin {int(d[0])}: {int(hist[d[0]])} counted, {int(want[d[0]])} keys belong there ({d.size} bins differ)")
    return bad


def check_buckets(keys, warm_lo, shift, hist, buckets, cap):
    """Bins 1 .. 2046: a bin with count <= cap holds exactly the multiset of its keys in its first ``count`` slots; a fuller one holds a
    sub-multiset of them in its ``cap`` slots.  Judged by bit patterns."""
    bad = []
    bits = f64_bits(np.asarray(keys, dtype=np.float64).reshape(-1))
    bins = warm_bin(bits, warm_lo, shift)
    hist = np.asarray(hist).astype(np.int64)
    bk = f64_bits(buckets).reshape(SEL_BINS, cap)
    order = np.argsort(bins, kind="stable")
    starts = np.searchsorted(bins[order], np.arange(SEL_BINS + 1))
    for b in range(1, SEL_BINS - 1):
        mine = np.sort(bits[order[starts[b]:starts[b + 1]]])
        cnt = int(hist[b])
        if cnt != mine.size:
            bad.append(f"bucket {b}: the histogram says {cnt}, {mine.size} keys belong there")
            continue
        got = np.sort(bk[b, :min(cnt, cap)])
        if cnt <= cap:
            if not np.array_equal(got, mine):
                bad.append(f"bucket {b}: its {cnt} slots do not hold the bin's keys")
        else:
            u, c = np.unique(got, return_counts=True)
            mu, mc = np.unique(mine, return_counts=True)
            pos = np.searchsorted(mu, u)
            ok = np.all(pos < mu.size) and np.all(mu[np.minimum(pos, mu.size - 1)] == u) and np.all(c <= mc[np.minimum(pos, mu.size - 1)])
            if not ok:
                bad.append(f"bucket {b} (full: {cnt} keys, cap {cap}): its slots are no sub-multiset of the bin's keys")
    return bad[:8]


# ------------------------------------------------------------------------------------------------ the oracle's figures
def oracle_levels(c, it, lam, initialize, n_max=None, m_max=None, lanes16=True, hop=False, reg=False):
    """``R.Levels`` of the fp64 NumPy oracle on case ``c`` for the quantities of this module: its own first trial through the layers
    above (fp64 sums of its own terms in slot order against the longdouble sums at its own trial states and weights), on top of
    ``R.oracle_levels`` (retract, step_fwd, last_hessian of a landmark-only call).  Asserts the conditions on the case: the first
    trial accepted with a margin, nothing where nothing is summed."""
    prior = c.prior() if reg else None
    lv = R.oracle_levels(c.args(), it, lam, initialize, hop=hop, prior=prior)
    o = lv.oracle
    dbg, out = o["dbg"], o["out"]
    tr = dbg["trials"][0]
    assert tr["residual"] < MARGIN * dbg["init_residual"], \
        f"a badly chosen case: the oracle's first trial {tr['residual']!r} is not {MARGIN} below its initial residual {dbg['init_residual']!r}"
    n_max, m_max = c.n if n_max is None else n_max, c.m if m_max is None else m_max
    sigma = o["sigma"]
    exact, figs = [], {}
    ch = chain_terms(out, c.t, c.cumrot, sigma, initialize, hop, prior if not initialize else None)
    nl = int(ch["long"].sum())
    ref = slot_sums(c.uv, tr["est"], dbg["w"], c.ii, ch, n_max, m_max, lanes16, nl)
    # the oracle's own sums, fp64, slot by slot
    order = sorted_order(c.ii)
    r = np.abs(c.uv - tr["est"])
    wt, raw = (r * dbg["w"][:, None]).sum(-1)[order], r.sum(-1)[order]
    no, nd = geometry(n_max, m_max, lanes16)
    pt = np.zeros(no + nd + nl)
    pn = np.zeros(no)
    for t in range(-(-c.m // TILE)):
        pt[t], pn[t] = wt[t * TILE:t * TILE + TILE].sum(), raw[t * TILE:t * TILE + TILE].sum()
    if not initialize:
        rp = np.abs(O.dynamics_residual(out, c.cumrot, c.t, initialize, hop=hop)) * np.sqrt(sigma)
        if reg:
            rp[:, 6] *= 1.0 / O.QUAT_COEFF
            pr = np.abs(O.prior_factor(out, prior[0], prior[1], vel_coeff=1.0)[0]).sum(-1)
        lidx = list(np.nonzero(ch["long"])[0])
        for i in range(c.n - 1):
            orb = rp[i, :6].sum()
            if ch["long"][i]:
                pt[no + nd + lidx.index(i)] = orb
                orb = 0.0
            pt[no + edge_slot(i, lanes16)] += orb + rp[i, 6]
        if reg:
            for j in range(c.n):
                pt[no + pose_slot(j, nd, lanes16)] += pr[j]
    figs.update(slot_figures(ref, pt, pn, nl, exact))
    mean, den = trial_mean(ref, c.n, c.m, initialize, reg)
    figs["mean"] = R.sums_figure(tr["residual"], mean, den)
    if not initialize:
        figs["retract"] = retract_figure(c.states, tr["dpose"], out, exact)
    assert not exact, exact
    units = dict(lv.units)
    units.update(R._units(figs))
    units.setdefault("part_long", 0.0)
    bad = {k: v for k, v in units.items() if not v <= R.K_CASE_MAX}
    assert not bad, f"a badly chosen case: the oracle's own figures {bad} exceed {R.K_CASE_MAX:g} x 2^-53"
    return R.Levels(units, o)
