"""The median select of a BA call (vinsat_amd/csrc/vba_select.hip, vba_select_body.h) in exact integer terms: which branch a key set
takes, and a model of every branch that can be broken on purpose.  NumPy and Python integers only, no GPU needed.

The keys are the 2 m values |du|, |dv| of a window in the device's (pose-sorted) row order.  They are non-negative doubles, so their
bit patterns order like the values and everything below works on ``uint64`` patterns.  ``lower_median`` is the one reference of the
GPU tests: the select is exact, so there is no tolerance anywhere but in ``sum_bound``.

Restated from vba_device.h (tests/test_select_reference_host.py holds them against hand-written key sets):
  sel_shift / sel_width   the six radix digits of the exact select: 10 + 11 + 11 + 11 + 11 + 9 bits from bit 62 down
  warm_bin                bin of a key in the warm histogram: 0 below ``lo``, 1 .. 2046 inside, 2047 above
  warm_range_start        ``lo`` for the median bits of the call in front (2^64 - 1: no range)
  SEL_BINS 2048, COUNT_LIMIT 1024 (a longer list is not ranked by counting), WARM_COUNT 192 (kWarmCount), SEL_ITEMS 8 (kSelItems)

Branches (``select_finish_list``).  Exact select, list = the keys that ``k_select_pass<2, true>`` appends: those that match the digits
known when it runs, 0 and 1 -- ``key >> sel_shift(1)`` = ``key >> LIST_SHIFT`` (42), the sign, the exponent and 10 bits of the mantissa.
(Digit 2 is histogrammed by the same pass, so 32 bits are KNOWN once it has run; the list is the wider set.)
  count              list of <= 1024 keys: ranked by counting
  digits             longer: digit 2 from the pass's histogram, then digits 3, 4, 5 over the list
Sharded mode (``predict_gathered``): the list has room for the 2 m_max keys of the rank's own slice and is filled from the gathered keys
of all ranks, so it can overflow (cnt > 2 m_local; entries beyond the capacity are dropped by the append):
  overflow-short     2 m_local < cnt <= 1024: digits 2 .. 5 over the gathered keys -- not a count over the truncated list
  overflow-long      cnt > 1024 and > 2 m_local: the same fallback
tests/test_gpu_sharded_stages.py runs all four on emulated ranks.
Warm select, list = the keys of the warm bin of the wanted rank:
  subbin             <= 1024 keys: the top 8 bits of the offset inside the bin split them over 256 sub-bins, one is ranked
  long-first-digit   more: the first 11-bit digit of the offset, and its sub-bin (<= 1024 keys) is ranked by counting
  long-radix         that sub-bin holds more than 1024 keys too: the remaining digits by radix
or a miss (the call repeats its select with the exact digits): ``no-range`` (lo = 2^64 - 1), ``below`` (bin 0), ``above`` (bin 2047),
``full`` (the bin holds more than ``list_cap`` keys: the bucket capacity with the inline select, 2 m_max otherwise), ``forced``.

``select_model`` walks the same branches on lists laid out as the kernels lay them out and takes ``faults``: the planted mistakes of
tests/test_select_reference_host.py.  Without a fault it returns ``lower_median`` on every input (asserted there).
"""
import numpy as np

LD = np.longdouble
SEL_BINS = 2048
COUNT_LIMIT = 1024
WARM_COUNT = 192
SEL_ITEMS = 8
SEL_ITEMS_BATCH = 32
NO_RANGE = (1 << 64) - 1
MASK64 = (1 << 64) - 1
LIST_SHIFT = 42                 # sel_shift(1): the compacted list of the exact select holds the keys that agree above this bit
MISSES = ("no-range", "below", "above", "full", "forced")
EXACT_BRANCHES = ("count", "digits")
GATHERED_BRANCHES = ("count", "digits", "overflow-short", "overflow-long")
WARM_BRANCHES = ("subbin", "long-first-digit", "long-radix")


def sel_shift(p):
    return (53, 42, 31, 20, 9, 0)[p]


def sel_width(p):
    return 10 if p == 0 else 9 if p == 5 else 11


def f64_bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1).view(np.uint64)


def bits_f64(b):
    return float(np.array([int(b)], dtype=np.uint64).view(np.float64)[0])


def lower_median(keys):
    """The lower median of ``keys`` (any shape), as a float: the element of rank (size - 1) // 2 of the sorted bit patterns."""
    b = f64_bits(keys)
    assert b.size and not (b >> np.uint64(63)).any(), "the keys are non-negative doubles"
    return bits_f64(np.sort(b)[(b.size - 1) // 2])


def warm_range_start(c_bits, shift):
    c_bits = int(c_bits)
    binades = 2046 >> (52 - shift)
    down = (binades + 1) // 2
    e = c_bits >> 52
    if e <= down or e >= 0x7FE:
        return NO_RANGE
    return c_bits - (down << 52)


def warm_bin(key_bits, lo, shift):
    k = np.asarray(key_bits, dtype=np.uint64)
    lo = np.uint64(lo)
    below = k < lo
    d = (np.where(below, lo, k) - lo) >> np.uint64(shift)
    return np.where(below, 0, np.where(d < 2046, d + np.uint64(1), 2047)).astype(np.int64)


def _resolve(hist, rank):
    """``select_resolve``: (bin of ``rank`` in the histogram, rank inside it, count of that bin)."""
    cum = np.cumsum(hist)
    b = int(np.searchsorted(cum, rank, side="right"))
    return b, int(rank - (cum[b] - hist[b])), int(hist[b])


def _neighbours(ranked, r):
    """How many of the neighbours of rank ``r`` in the sorted keys ``ranked`` (the set the last step of the select ranks) exist and
    differ from it: 2 inside a set of different keys, so that a rank off by one either way gives another value."""
    ranked = np.sort(np.asarray(ranked, dtype=np.uint64))
    return int(r > 0 and ranked[r - 1] != ranked[r]) + int(r + 1 < ranked.size and ranked[r + 1] != ranked[r])


# ------------------------------------------------------------------------------------------------ predictors
def predict_exact(keys, m_max):
    """The exact select on ``keys``: dict with ``cnt`` (the list: keys agreeing with the median above bit ``LIST_SHIFT``), ``rank`` (the
    wanted rank among them), ``branch`` (``count`` / ``digits``), ``key`` and ``neighbours`` (see ``_neighbours``).  All keys are the
    handle's own here, at most 2 m_max, so the list cannot overflow (asserted); on a sharded handle it can: ``predict_gathered``,
    tests/test_gpu_sharded_stages.py."""
    p = predict_gathered(keys, m_max)
    assert p["cnt"] <= 2 * m_max, "more keys than the handle has rows for: this is a gathered key set (predict_gathered)"
    return p


def predict_gathered(keys, m_local, shift=LIST_SHIFT):
    """The exact select over the 2 m gathered ``keys`` of all ranks (without the +inf padding) on a rank whose handle was made for
    ``m_local`` rows: dict as ``predict_exact``, ``branch`` one of ``GATHERED_BRANCHES``.  ``shift``: the bit above which the list's keys
    agree -- 42 is what the kernel matches on, 31 the other reading of its comment; the sharded cases are built so that both give the
    same list (tests/test_sharded_stage_cases_host.py)."""
    b = f64_bits(keys)
    s = np.sort(b)
    want = (b.size - 1) // 2
    pre = s >> np.uint64(shift)
    lo = int(np.searchsorted(pre, pre[want], side="left"))
    cnt = int(np.searchsorted(pre, pre[want], side="right")) - lo
    cap = 2 * int(m_local)
    if cnt <= COUNT_LIMIT:
        branch = "count" if cnt <= cap else "overflow-short"
    else:
        branch = "digits" if cnt <= cap else "overflow-long"
    return dict(cnt=cnt, rank=want - lo, branch=branch, key=bits_f64(s[want]), neighbours=_neighbours(s[lo:lo + cnt], want - lo))


def gathered_model(abs_all, m_total, m_local, faults=()):
    """The select of stage 2 on the gathered buffer ``abs_all`` (the ranks' slots in rank order, each padded with +inf to 2 m_pad keys) as
    the kernels run it: the rank wanted is that of the 2 ``m_total`` real keys, the list is truncated at 2 ``m_local`` entries, an
    overflowed list goes to the digits over the whole buffer.  Returns the median as a float (None where a broken model finds none).
    ``faults``: ``rank_from_count_all`` (the rank taken from the buffer's length, padding included), ``truncated_list_ranked`` (a list
    of cnt <= 1024 entries ranked by counting although only its first 2 m_local were written: the others read as zero bits)."""
    bits = [int(x) for x in f64_bits(abs_all)]
    count = len(bits) if "rank_from_count_all" in faults else 2 * int(m_total)
    want = (count - 1) // 2
    a = np.array(bits, dtype=np.uint64)
    s = np.sort(a)
    pre = int(s[want]) >> LIST_SHIFT
    r = want - int((a >> np.uint64(LIST_SHIFT) < np.uint64(pre)).sum())
    lst = [k for k in bits if k >> LIST_SHIFT == pre]
    cap = 2 * int(m_local)
    if len(lst) > cap:
        if "truncated_list_ranked" in faults and len(lst) <= COUNT_LIMIT:
            out = _rank_by_counting(lst[:cap] + [0] * (len(lst) - cap), r, ())
            return None if out is None else bits_f64(out)
        lst = bits                                                    # the fallback: digits over every gathered key
    out = finish_list(lst, r, 0) if len(lst) <= cap else _radix(lst, r, pre, [(sel_shift(p), sel_width(p)) for p in (2, 3, 4, 5)])
    return None if out is None else bits_f64(out)


def predict_warm(keys, warm_lo, shift, list_cap, force_miss=False):
    """The warm select on ``keys`` binned from ``warm_lo`` with bins of 2^shift: dict with ``bin``, ``in_bin``, ``rank`` (inside the bin),
    ``hit``, ``miss`` (None or the reason, in the order ``front_resolve`` tests them) and, on a hit, ``branch``, ``sub_cnt`` (the keys of
    the sub-bin that is ranked last: of the 256 of a short list, of the first digit's 2048 of a long one), ``sub_rank`` (the wanted rank
    inside it) and ``neighbours`` (see ``_neighbours``) of the wanted key there."""
    b = f64_bits(keys)
    bins = warm_bin(b, warm_lo, shift)
    hist = np.bincount(bins, minlength=SEL_BINS)
    bn, rank, in_bin = _resolve(hist, (b.size - 1) // 2)
    miss = None
    if int(warm_lo) == NO_RANGE:
        miss = "no-range"
    elif bn == 0:
        miss = "below"
    elif bn == 2047:
        miss = "above"
    elif in_bin > list_cap:
        miss = "full"
    elif force_miss:
        miss = "forced"
    out = dict(bin=bn, in_bin=in_bin, rank=rank, hit=miss is None, miss=miss, branch=None, sub_cnt=None, sub_rank=None, neighbours=None)
    if miss is None:
        base = int(warm_lo) + ((bn - 1) << shift)
        mine = b[bins == bn]
        width = 8 if in_bin <= COUNT_LIMIT else 11
        rel = ((mine - np.uint64(base)) >> np.uint64(shift - width)).astype(np.int64)
        d, r, sub = _resolve(np.bincount(rel, minlength=1 << width), rank)
        out.update(sub_cnt=sub, sub_rank=r, neighbours=_neighbours(mine[rel == d], r))
        out["branch"] = "subbin" if width == 8 else "long-first-digit" if sub <= COUNT_LIMIT else "long-radix"
    return out


def sum_bound(m, nblk):
    """Relative bound on the device's sum of the 2 m keys of a window (``sc.sum_in``, and the init residual of a landmark-only BA
    call formed from it) against the exact sum, ``nblk`` = ceil(m_max / 256) block partials.

    The terms are non-negative, so a sum evaluated in any order with d roundings on the longest path from a term to the result is
    within d u (1 + O(d u)) of the exact sum, u = 2^-53.  The device's order (``block_sum``, vba_device.h):
      k_obs_residual   |du| + |dv| of a row: 1 rounding; ``wave_sum``: a butterfly of 6 levels, 6 roundings; thread 0 adds the 4 wave
                       partials to 0.0: the first addition is exact, 3 roundings.  ``block_sum<256>`` is 6 + 3 = 9 deep.
      k_select_pass<1> thread t adds the partials t, t + 256, ... to 0.0: ceil(nblk / 256) - 1 roundings; ``block_sum<256>`` again: 9.
      the accept test  (sum + 0) / denominator: 1 rounding (the pose-chain term of a landmark-only call is an exact 0.0).
    Longest path: 2 x 9 + ceil(nblk / 256) + 1, where the 10 of the bar stands.  The bar keeps the 10: it covers the second-order terms
    ((1 + u)^28 - 1 < 28.01 u) and is a bound either way, not a measurement.  The depth does not grow with ``m``: the partials are
    summed by a tree; ``m`` only has to fit the blocks."""
    assert 0 < int(m) <= 256 * int(nblk), "the rows of a window fit the blocks of its handle"
    return (2 * 9 + -(-int(nblk) // 256) + 10) * 2.0 ** -53


def exact_sum(keys):
    return np.asarray(keys, dtype=np.float64).reshape(-1).astype(LD).sum()


# ------------------------------------------------------------------------------------------------ the model
def _rank_by_counting(lst, want, faults):
    """Rank each key of ``lst`` (Python ints) by counting, ties broken by position; None if no key has the wanted rank."""
    n = len(lst) - 1 if "count_drops_last" in faults else len(lst)
    a = np.array(lst[:n], dtype=np.uint64)
    out = None
    for q in range(n):
        below = int((a < a[q]).sum())
        if "tie_by_value" not in faults:
            below += int((a[:q] == a[q]).sum())
        if below == want:
            out = int(a[q])
    return out


def _radix(lst, want, prefix, shifts_widths, faults=()):
    """Digits over ``lst`` from the given (shift, width) pairs; ``prefix`` = the bits above the first digit."""
    a = np.array(lst, dtype=np.uint64)
    rank = want
    for sh, wd in shifts_widths:
        sel = a[(a >> np.uint64(sh + wd)) == np.uint64(prefix)]
        d, rank, _c = _resolve(np.bincount(((sel >> np.uint64(sh)) & np.uint64((1 << wd) - 1)).astype(np.int64), minlength=1 << wd), rank)
        prefix = (prefix << wd) | d
    return prefix


def finish_list(lst, want, mode, warm_base=0, shift=44, faults=()):
    """``select_finish_list`` on a list of bit patterns (Python ints, the order the kernel left them in): the key of rank ``want``, or
    None where the (broken) model finds none.  mode 0: the keys agree above bit ``LIST_SHIFT``; 1: the keys of one warm bin."""
    cnt = len(lst)
    limit = COUNT_LIMIT + 2 if "count_limit_high" in faults else COUNT_LIMIT
    if mode == 1 and "warm_base_bin" in faults:
        warm_base = (warm_base + (1 << shift)) & MASK64              # lo + (bin << shift): the bin index not moved down by one
    if mode == 1 and cnt <= limit:
        loaded = lst[:COUNT_LIMIT]                                    # (four entries per thread are all that is loaded)
        sh = shift - 8
        sb = [(((k - warm_base) & MASK64) >> sh) & 255 for k in loaded]
        tb, r, _c = _resolve(np.bincount(sb, minlength=256), want) if want < len(loaded) else (None, 0, 0)
        return _rank_by_counting([k for k, s in zip(loaded, sb) if s == tb], r, faults)
    if mode == 0 and cnt <= limit:
        return _rank_by_counting(lst[:COUNT_LIMIT], want, faults)
    if mode == 1:
        rem = shift - 11
        rel = [(k - warm_base) & MASK64 for k in lst]
        d, r, sub = _resolve(np.bincount([(x >> rem) & 2047 for x in rel], minlength=SEL_BINS), want)
        if sub <= COUNT_LIMIT:
            return _rank_by_counting([k for k, x in zip(lst, rel) if (x >> rem) == d], r, faults)
        if "rank_not_rebased" in faults:
            r = want
        plan = []
        while rem > 0:
            wd = min(rem, 11)
            rem -= wd
            plan.append((rem, wd))
        try:
            return (warm_base + _radix(rel, r, d, plan)) & MASK64
        except IndexError:                                            # (a rank beyond the sub-bin: nothing is found)
            return None
    prefix = lst[0] >> LIST_SHIFT if lst else 0
    return _radix(lst, want, prefix, [(sel_shift(p), sel_width(p)) for p in (2, 3, 4, 5)])


def select_model(slot_keys, m, m_max, warm=None, items=SEL_ITEMS, faults=()):
    """The select of one window as the kernels run it.  ``slot_keys``: the 2 m_max doubles of the window's key slot in device order (what
    lies behind 2 m is whatever an earlier window left: the select must not look at it).  ``warm``: None for the exact select, else
    dict(lo, shift, list_cap).  Returns the median as a float, or None where a broken model finds no key / a warm select misses."""
    bits = [int(x) for x in f64_bits(slot_keys)]
    count = 2 * m_max if "reads_m_max" in faults else 2 * m
    keys = bits[:count]
    if "block_tail_dropped" in faults:                                # the last key pair of every full block of 256 x items keys
        per = 256 * items
        keys = [k for i, k in enumerate(keys) if not (i % per >= per - 2 and (i // per + 1) * per <= count)]
    want = (count // 2) if "upper_median" in faults else (count - 1) // 2
    a = np.array(keys, dtype=np.uint64)
    if warm is None:
        s = np.sort(a)
        pre = int(s[min(want, s.size - 1)]) >> LIST_SHIFT
        lst = [k for k in keys if k >> LIST_SHIFT == pre]
        if "list_cap_short" in faults and len(lst) >= 2 * m_max:
            lst[2 * m_max - 1] = 0                                    # the guard `base + off < 2 m_max` one too tight: the slot is never written
        r = want - int((a >> np.uint64(LIST_SHIFT) < np.uint64(pre)).sum())
        out = finish_list(lst, r, 0, faults=faults)
    else:
        lo, shift = int(warm["lo"]), int(warm["shift"])
        bins = warm_bin(a, lo, shift)
        bn, r, in_bin = _resolve(np.bincount(bins, minlength=SEL_BINS), want)
        if lo == NO_RANGE or bn < 1 or bn > 2046 or in_bin > warm["list_cap"]:
            return None
        lst = [k for k, b in zip(keys, bins) if b == bn]
        out = finish_list(lst, r, 1, lo + ((bn - 1) << shift), shift, faults)
    return None if out is None else bits_f64(out)
