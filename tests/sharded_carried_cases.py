"""Cases and references of the exchange-by-exchange tests of the sharded carried-keys protocol (tests/test_gpu_sharded_carried.py; the
conditions on the cases and the planted faults: tests/test_sharded_carried_host.py).  NumPy only.

Windows: ``sharded_stage_cases.slices()`` / ``head(R + 1)`` / ``rejecting(conf)`` and, for the misses (``band_case``, ``leaving_case``):
  overflow-one-rank   R = 3, bucket cap 8 on every rank, 90 rows: 10 / 8 / 4 keys of the median's bin: rank 0 alone overflows
  overflow-twin       8 / 8 / 4 keys: exactly the cap on the fullest ranks: a hit on a bin of 20 keys
  long-bin            R = 5, default cap 256, 1500 rows (two observation blocks per rank): 205 keys per rank = 1025 > 1024 over all
                      ranks, no bucket above its cap.  Five ranks were chosen over a handle big enough for cap 512.
  long-twin           205, 205, 205, 205, 204 keys = 1024: a hit on the longest list the front lets through
  leaving             R = 3, 96 rows measured 40 px off per pose, from lamda = 1e-4: the median falls to under a pixel, below c / 16
                      where the binned range of shift 44 begins (bin 0)

The model of ``k_sh_front`` (vinsat_amd/csrc/vba_shard.hip): ``front_model`` takes the gathered slots of exchange A and returns what the
kernel resolves and decides, integers exactly and the two residuals in fp64 in the kernel's own order (per thread t: over the ranks,
then over the blocks b = t, t + 256, ...; the pose-chain blocks from slot 0 only; ``wave_sum``; ((r0 + r1) + r2) + r3)."""
from dataclasses import replace

import numpy as np

import dynamics_cases as D
import sharded_stage_cases as C
import trial_reference as TR

SHIFT = 44
SEL_BINS = 2048
LIST_MAX = 1024
CALL_SEQ = ((0, True), (1, True), (12, False), (13, False))     # landmark-only calls, then full calls; from lamda = D.LAM_INIT
LAM0 = D.LAM_INIT
MAX_WORLD = 8
REASONS = ("forced", "overflow", "long", "leaving")


# ------------------------------------------------------------------------------------------------ layout of the exchanges
def len_a(nblk_obs, trial_stride):
    return (1024 + nblk_obs + trial_stride + 3) & ~3


def len_b(bucket_cap):
    return (bucket_cap + 4) & ~3


def split_a(slot, nblk_obs, trial_stride):
    """(hist [2048] uint32, part_next [nblk_obs], part_trial [trial_stride]) of one rank's slot of exchange A (doubles)."""
    slot = np.ascontiguousarray(slot, dtype=np.float64)
    hist = slot[:1024].view(np.uint32).copy()
    return hist, slot[1024:1024 + nblk_obs].copy(), slot[1024 + nblk_obs:1024 + nblk_obs + trial_stride].copy()


def pack_a(hist, part_next, part_trial):
    h = np.ascontiguousarray(hist, dtype=np.uint32)
    assert h.size == SEL_BINS
    out = np.zeros(len_a(len(part_next), len(part_trial)))
    out[:1024] = h.view(np.float64)
    out[1024:1024 + len(part_next)] = part_next
    out[1024 + len(part_next):1024 + len(part_next) + len(part_trial)] = part_trial
    return out


# ------------------------------------------------------------------------------------------------ the model of k_sh_front
def _thread_sums(slots, off, count, ranks):
    """Per thread t of 256: over the ranks q, then over b = t, t + 256, ...: s += slot_q[off + b] (fp64, from 0.0)."""
    s = np.zeros(256)
    for q in ranks:
        for b0 in range(0, count, 256):
            seg = np.asarray(slots[q][off + b0:off + min(count, b0 + 256)], dtype=np.float64)
            s[:seg.size] = s[:seg.size] + seg
    return s


def _block_total(per_thread):
    w = [C._wave_sum(per_thread[64 * k:64 * k + 64]) for k in range(4)]
    return ((w[0] + w[1]) + w[2]) + w[3]


def front_sums(slots, nblk_obs, nblk_chain, faults=()):
    """(sum_next, sum_trial) of the gathered slots as ``k_sh_front`` adds them up: the observation blocks of every rank, the ``nblk_chain``
    pose-chain (and long-edge) blocks of slot 0 alone.  Faults: ``chain_from_every_rank`` (the pose-chain part added R times)."""
    R = len(slots)
    s_next = _thread_sums(slots, 1024, nblk_obs, range(R))
    s_trial = _thread_sums(slots, 1024 + nblk_obs, nblk_obs, range(R))
    # (the accumulator that holds the observation part takes the pose-chain blocks of slot 0 behind it, in block order)
    st = s_trial.copy()
    src = range(R) if "chain_from_every_rank" in faults else [0]
    for q in src:
        for b0 in range(0, nblk_chain, 256):
            seg = np.asarray(slots[q][1024 + 2 * nblk_obs + b0:1024 + 2 * nblk_obs + min(nblk_chain, b0 + 256)], dtype=np.float64)
            st[:seg.size] = st[:seg.size] + seg
    return _block_total(s_next), _block_total(st)


def residuals(sum_in, sum_pred, sum_trial, n, m_total, initialize):
    """(init_residual, trial_residual) of ``decide_finish`` without a prior, fp64 in its order."""
    denom = 2.0 * float(m_total) + (6.0 if initialize else 7.0) * float(n - 1) + 0.0
    return (sum_in + (0.0 if initialize else sum_pred) + 0.0) / denom, (sum_trial + 0.0) / denom


def front_resolve(slots, m_total, bucket_cap, warm_lo, forced=False, faults=()):
    """The resolve step: dict with ``hist`` (the R histograms added up), ``bin``, ``rank`` (of the global lower median inside the bin),
    ``in_bin``, ``over`` (ranks whose bucket of that bin overflowed), ``hit`` and ``reason`` (None on a hit; else the FIRST of
    ``leaving`` / ``long`` / ``overflow`` / ``forced`` that holds -- ``reasons`` has all of them).
    Faults: ``drop_last_rank`` (the histogram summed over R - 1 ranks), ``cap_ge`` (count >= cap is an overflow)."""
    R = len(slots)
    hs = [np.ascontiguousarray(s[:1024], dtype=np.float64).view(np.uint32).astype(np.int64) for s in slots]
    hist = np.zeros(SEL_BINS, dtype=np.int64)
    for q in range(R - 1 if "drop_last_rank" in faults else R):
        hist += hs[q]
    want = (2 * int(m_total) - 1) // 2
    cum = np.cumsum(hist)
    b = int(np.searchsorted(cum, want, side="right"))
    b = min(b, SEL_BINS - 1)
    rank = want - (int(cum[b - 1]) if b > 0 else 0)
    in_bin = int(hist[b])
    over = [q for q in range(R) if (hs[q][b] >= bucket_cap if "cap_ge" in faults else hs[q][b] > bucket_cap)]
    reasons = []
    if int(warm_lo) == (1 << 64) - 1 or not 1 <= b <= SEL_BINS - 2:
        reasons.append("leaving")
    if in_bin > LIST_MAX:
        reasons.append("long")
    if over:
        reasons.append("overflow")
    if forced:
        reasons.append("forced")
    return dict(hist=hist, own=hs, bin=b, rank=rank, in_bin=in_bin, over=over, hit=not reasons, reason=reasons[0] if reasons else None,
                reasons=reasons)


def front_model(slots, m_total, bucket_cap, warm_lo, nblk_obs, nblk_chain, n, initialize, sum_in, sum_pred, forced=False, faults=()):
    """Everything ``k_sh_front`` learns from the gathered exchange A ``slots`` (one array of lenA doubles per rank).  ``initialize``,
    ``sum_in``, ``sum_pred``, ``nblk_chain``: of the DECIDED call (the one whose trial wrote these slots: nblk_dyn, plus nblk_long when
    it was a full call).  Returns ``front_resolve``'s dict with ``sum_in`` (the NEXT call's: sum |r| over all ranks), ``init_residual``,
    ``trial_residual``."""
    d = front_resolve(slots, m_total, bucket_cap, warm_lo, forced, faults)
    s_next, s_trial = front_sums(slots, nblk_obs, nblk_chain, faults)
    d["sum_in"] = s_next
    d["init_residual"], d["trial_residual"] = residuals(sum_in, sum_pred, s_trial, n, m_total, initialize)
    return d


def expected_bucket(own_keys, warm_lo, b):
    """The sorted bit patterns of a rank's keys that fall into bin ``b``."""
    bits = TR.f64_bits(np.asarray(own_keys, dtype=np.float64).reshape(-1))
    return np.sort(bits[TR.warm_bin(bits, warm_lo, SHIFT) == b])


def own_hist(own_keys, warm_lo):
    return np.bincount(TR.key_bins(own_keys, 2, warm_lo, SHIFT), minlength=SEL_BINS).astype(np.int64)


# ------------------------------------------------------------------------------------------------ layers c and d as comparisons
def check_bucket(sent, own_keys, warm_lo, b, word):
    """Exchange B as a rank sent it, [count, keys ...], against its next keys ``own_keys``, the resolved bin ``b`` and its own histogram
    word of that bin: [] or what is wrong."""
    want = expected_bucket(own_keys, warm_lo, b)
    cnt = int(sent[0])
    if sent[0] != word or cnt != want.size:
        return [f"bucket count {sent[0]!r}, its histogram word of bin {b} is {int(word)}, {want.size} of its keys belong there"]
    if not np.array_equal(np.sort(TR.f64_bits(np.asarray(sent[1:1 + cnt], dtype=np.float64))), want):
        return [f"the bucket it sent does not hold its keys of bin {b}"]
    return []


def check_median(c_obs, keys_of_all_ranks):
    """``c_obs`` against the lower median of the concatenated keys of all ranks: [] or what is wrong."""
    import select_reference as S
    allk = np.concatenate([np.asarray(q, dtype=np.float64).reshape(-1) for q in keys_of_all_ranks])
    med = S.lower_median(allk)
    return [] if c_obs == med else [f"c_obs {c_obs!r}, the lower median of the {allk.size} keys of all ranks is {med!r}"]


def check_key_exchange(sent, own_keys, ii, m_pad):
    """A key exchange as a rank sent it: its keys in device order, then +inf up to 2 m_pad."""
    import select_cases as SC
    bad = []
    m_r = np.asarray(ii).size
    if np.asarray(sent).size != 2 * m_pad:
        return [f"a key exchange of {np.asarray(sent).size} doubles, the slot has {2 * m_pad}"]
    if not np.array_equal(TR.f64_bits(sent[:2 * m_r]), TR.f64_bits(SC.device_order(own_keys, ii))):
        bad.append("the key exchange does not hold its keys in device order")
    if not np.all(np.isposinf(sent[2 * m_r:])):
        bad.append("the padding of its key slot is not +inf")
    return bad


# ------------------------------------------------------------------------------------------------ the exchange pattern
def pattern(carried, missed, stalled, n_trials, lenA, lenB, n, m_pad):
    """Element counts of the all-gathers of ONE ``vba_sh_call``, in order: B, C, A on carried keys (keys, C, A without); a missed select
    repeats the call without carried keys; a stalled call gathers 2 doubles per LM trial and A once more at its end."""
    pc = 27 * n + 2
    out = [lenB, pc, lenA] if carried else [2 * m_pad, pc, lenA]
    if missed:
        out += [2 * m_pad, pc, lenA]
    if stalled:
        out += [2] * n_trials + [lenA]
    return out


# ------------------------------------------------------------------------------------------------ block sums of a rank
def slot_bars(c, rows, est, weight, out_states, sigma, initialize, m_pad):
    """(ref, bars, nblk_long) of a rank's block sums: ``trial_reference.slot_sums`` of its rows ``c[rows]`` at the trial states
    ``out_states`` and, per quantity, K = max(16, 4 x the figure of fp64 NumPy summing the same terms slot by slot), as
    tests/test_gpu_trial_paths.py sets its bars (``trial_reference.oracle_levels``, evaluated here at the judged side's states)."""
    from oracle import ba_oracle as O
    sub = C.take_rows(c, rows)
    ch = TR.chain_terms(out_states, c.t, c.cumrot, sigma, initialize)
    nl = int(ch["long"].sum())
    ref = TR.slot_sums(sub.uv, est, weight, sub.ii, ch, c.n, m_pad, True, nl)
    wt, raw = TR.row_terms(sub.uv, est, weight, sub.ii)
    no, nd = TR.geometry(c.n, m_pad, True)
    pt, pn = np.zeros(no + nd + nl), np.zeros(no)
    for t in range(-(-sub.m // TR.TILE)):
        pt[t] = wt.astype(np.float64)[t * TR.TILE:t * TR.TILE + TR.TILE].sum()
        pn[t] = raw.astype(np.float64)[t * TR.TILE:t * TR.TILE + TR.TILE].sum()
    if not initialize:
        rp = np.abs(O.dynamics_residual(out_states, c.cumrot, c.t, initialize)) * np.sqrt(sigma)
        lidx = list(np.nonzero(ch["long"])[0])
        for i in range(c.n - 1):
            orb = rp[i, :6].sum()
            if ch["long"][i]:
                pt[no + nd + lidx.index(i)] = orb
                orb = 0.0
            pt[no + TR.edge_slot(i, True)] += orb + rp[i, 6]
    exact = []
    own = TR.slot_figures(ref, pt, pn, nl, exact)
    assert not exact, exact
    bars = {k: max(16.0, 4.0 * float(np.max(v) / TR.U)) if np.size(v) else 16.0 for k, v in own.items()}
    return ref, bars, nl


def with_states(c, states):
    return replace(c, states=np.asarray(states, dtype=np.float64).copy())


# ------------------------------------------------------------------------------------------------ what the rank processes run
def _steps(calls):
    return [("step", it, init) for it, init in calls]


def case_of(name, world):
    """(case, bucket cap or 0, forced miss) of scenario ``name``."""
    base = name.split("/")[0]
    if base in BAND or base == "leaving":
        c, R, cap, _per = leaving_case() if base == "leaving" else band_case(base)
        assert R == world
        return c, cap, False
    if base == "head":
        return C.head(world + 1), 0, False
    if base.startswith("rejecting-"):
        return C.rejecting(float(base.split("-")[1])), 0, False
    return C.slices(), 0, base == "forced"


def scenarios(world):
    """name -> list of operations of every rank: ("step", iter, initialize) = one ``vba_sh_call``, ("sched", calls) = one
    ``vba_sh_run_schedule``, ("reupload",) = the rows split the other way round on the live handles, states set again."""
    s = {}
    if world in (1, 2, 3):
        s["slices/step"] = _steps(CALL_SEQ)
        s["head/step"] = _steps(CALL_SEQ)
        s["slices/chain"] = [("sched", CALL_SEQ)]
        s["slices/chain2"] = [("sched", CALL_SEQ[:2]), ("sched", CALL_SEQ[2:])]
        s["forced/step"] = _steps(CALL_SEQ[:3])
    if world in (2, 3):
        s["slices/reupload"] = _steps(CALL_SEQ[:2]) + [("reupload",)] + _steps(CALL_SEQ[:2])
    if world == 3:
        for conf in ("2.2", "3"):
            s[f"rejecting-{conf}/step"] = _steps(CALL_SEQ[:2])
            s[f"rejecting-{conf}/chain"] = [("sched", CALL_SEQ[:2])]
    for name, v in list(BAND.items()) + [("leaving", (3,))]:
        if v[0] == world:
            s[f"{name}/step"] = _steps(CALL_SEQ[:2])
    return s


def lam0_of(name):
    """The damping a scenario starts from (1e-4, the driver's first: the rejecting windows; ``leaving``, whose poses must follow their rows)."""
    return 1e-4 if name.startswith(("rejecting-", "leaving")) else LAM0


def split_bounds(m, world, resplit):
    """Row bounds of the ranks: ``shard_bounds``, or (``resplit``) rank 0 a row fewer and rank 1 a row more."""
    b = np.asarray(C.bounds(m, world)).copy()
    if resplit:
        b[1] -= 1
    return b


# ------------------------------------------------------------------------------------------------ the miss windows
# name -> (ranks, bucket cap or 0 = the default 256, rows per rank, keys of the band per rank)
BAND = {"overflow-one-rank": (3, 8, 30, (10, 8, 4)), "overflow-twin": (3, 8, 30, (8, 8, 4)),
        "long-bin": (5, 0, 300, (205, 205, 205, 205, 205)), "long-twin": (5, 0, 300, (205, 205, 205, 205, 204))}
BAND_REASON = {"overflow-one-rank": "overflow", "overflow-twin": None, "long-bin": "long", "long-twin": None, "leaving": "leaving"}
OFFSET, JITTER = 2.7, 1e-7
PIVOT = OFFSET + 0.003          # the first call's median: 0.003 px above the band, inside one warm bin of 2^-7 px with it
FAR = 6.0                       # the other component of a one-key copy
MOVERS, MOVER_BIAS = 4, 6.0
LEAVING_ROWS, LEAVING_BIAS = 32, 40.0
_BAND = {}


def _mags(rng, k, lo, hi):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), (k, 2))) * rng.choice([-1.0, 1.0], (k, 2))


def band_case(name):
    """A window whose SECOND call (carried keys) finds a band of tied keys in the bin of the global median, so many per rank as ``BAND``
    says.  Built like ``select_cases._repeated``: the band is ONE row of pose 0 repeated without weight and measured 2.7 px off (+- 1e-7;
    a one-key copy has its other component at 6 px); pose 0 has no weighted row, so it stays where it is and the copies keep their keys
    on every call.  The median's own bits start a warm bin, so the first call's median is made a key of its own -- the pivot, one more
    copy at 2.703 px with exactly m - 1 keys below it -- and four rows of pose 8, alone on their pose and measured 6 px off, make that
    pose follow them: their eight keys fall from above the pivot to below the band, and the second call wants the band's eighth key
    from the top, in the bin that ends at the pivot (0.0078 px wide at shift 44).  The other rows come in pairs measured off in
    opposite directions (below 2 px / above 3.5 px); copies without weight at 0.5 / 9 px settle the count.  Rows are not shuffled:
    rank r holds its share of the band.  Returns (case, ranks, cap, keys of the band per rank)."""
    if name in _BAND:
        return _BAND[name]
    import select_cases as SC
    R, cap, m_r, per_rank = BAND[name]
    rng = np.random.default_rng(9100 + sorted(BAND).index(name))
    p = SC.pool()
    own0 = int(np.nonzero(p.ii == 0)[0][0])
    own8 = np.nonzero(p.ii == 8)[0][:MOVERS]
    others = rng.permutation(np.nonzero((p.ii != 0) & (p.ii != 8))[0])
    m = R * m_r
    plan, n_pairs = [], 0
    for r in range(R):
        g = (per_rank[r] + 1) // 2
        special = 1 + MOVERS if r == R - 1 else 0
        left = m_r - g - special
        fill = 2 + left % 2
        plan.append((g, special, (left - fill) // 2, fill))
        n_pairs += (left - fill) // 2
    need = m - 1 - sum(per_rank)                    # keys below the pivot that the pairs and the fillers must supply
    n_fill = sum(q[3] for q in plan)
    nb = min(n_pairs, max(0, (need - n_fill) // 4))
    rest = need - 4 * nb
    assert 0 <= rest <= 2 * n_fill, (name, need, nb, n_fill)
    take, off, conf = [], [], []
    used = pairs_seen = 0
    for r, (g, special, pairs, fill) in enumerate(plan):
        band = np.full((g, 2), OFFSET) + rng.uniform(-JITTER, JITTER, (g, 2))
        if per_rank[r] % 2:
            band[-1, 1] = FAR
        fl = np.full((fill, 2), 9.0)
        for q in range(fill):
            k = min(2, rest)
            fl[q, :k] = 0.5
            rest -= k
        below = np.array([pairs_seen + q < nb for q in range(pairs)])
        pairs_seen += pairs
        half = np.where(below[:, None], _mags(rng, pairs, 0.3, 2.0), _mags(rng, pairs, 3.5, 20.0))
        rows = others[used:used + pairs]
        used += pairs
        take += [np.full(g + fill, own0), rows, rows]
        off += [band, fl, half, -half]
        conf += [np.zeros(g + fill), p.conf[rows], p.conf[rows]]
        if special:
            take += [np.full(1, own0), own8]
            off += [np.array([[PIVOT, FAR]]), MOVER_BIAS + rng.normal(0.0, 0.05, (MOVERS, 2))]
            conf += [np.zeros(1), p.conf[own8]]
    assert rest == 0
    c = SC._build(name, np.concatenate(take), np.concatenate(off), np.concatenate(conf))
    assert c.m == m
    _BAND[name] = (c, R, cap, per_rank)
    return _BAND[name]


def leaving_case(R=3):
    """``LEAVING_ROWS`` rows per rank, every row of a pose measured 40 px off in one direction (+- 0.05): the poses follow their rows, the
    oracle accepts the step, and the median falls from 40 px to a fraction of a pixel -- below c / 16, where the 2046 warm bins of
    shift 44 begin: the second call's median lies in bin 0."""
    key = ("leaving", R)
    if key not in _BAND:
        import select_cases as SC
        rng = np.random.default_rng(9200)
        p = SC.pool()
        m = LEAVING_ROWS * R
        take = rng.permutation(p.m)[:m]
        _BAND[key] = (SC._build("leaving", take, LEAVING_BIAS + rng.normal(0.0, 0.05, (m, 2))), R, 0, ())
    return _BAND[key]


def band_conditions(name):
    """What the oracle's keys say about ``band_case(name)`` / ``leaving_case()``: dict with ``trials`` of its landmark-only call, the
    first median, ``bin`` of the second call's median under the first one's range, ``in_bin`` and ``per_rank`` keys of that bin."""
    import select_cases as SC
    import select_reference as S
    from oracle import ba_oracle as O
    c, R, _cap, _per = leaving_case() if name == "leaving" else band_case(name)
    k0 = SC.oracle_keys(c)
    out, _lam, _h, ntr = O.ba_iteration(CALL_SEQ[0][0], c.states, c.cumrot, c.uv, c.xyz, c.ii, c.t, c.K, c.conf, lam0_of(name), initialize=True)
    k1 = SC.oracle_keys(c, out)
    med0, med1 = S.lower_median(k0), S.lower_median(k1)
    lo = TR.warm_range_start(int(TR.f64_bits([med0])[0]), SHIFT)
    b = int(TR.warm_bin(TR.f64_bits([med1]), lo, SHIFT)[0])
    per = [int((TR.warm_bin(TR.f64_bits(k1[C.rank_rows(c, R, r)].reshape(-1)), lo, SHIFT) == b).sum()) for r in range(R)]
    return dict(trials=ntr, med0=med0, med1=med1, bin=b, in_bin=sum(per), per_rank=per, m=c.m)
