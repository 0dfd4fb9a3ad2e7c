"""tests/select_reference.py and tests/select_cases.py on the CPU: the restated bin functions and the predictors on hand-written key
sets with known answers, the conditions on the cases (every case lands in the branch it was made for, with the oracle's keys -- the GPU
test repeats the assertion on the device's own keys), and the planted faults: for each broken model of the select, a named case whose
median comes out as another key (or as none)."""
import numpy as np
import pytest

import select_cases as C
import select_reference as S

BITS_1 = int(S.f64_bits([1.0])[0])


def _f(bits):
    return np.array(bits, dtype=np.uint64).view(np.float64)


# ------------------------------------------------------------------------------------------------ restated device functions
def test_digits_cover_the_63_key_bits():
    assert [S.sel_shift(p) for p in range(6)] == [53, 42, 31, 20, 9, 0]
    assert sum(S.sel_width(p) for p in range(6)) == 63
    for p in range(5):
        assert S.sel_shift(p) == S.sel_shift(p + 1) + S.sel_width(p + 1)
    assert (S.SEL_BINS, S.COUNT_LIMIT, S.WARM_COUNT, S.SEL_ITEMS) == (2048, 1024, 192, 8)


def test_warm_range_and_bins_on_known_values():
    # 2046 bins of 2^44 are 7 binades, 4 of them below the median: [c / 16, ...); 2^43: [c / 4, ...); 2^42: one binade, [c / 2, ...)
    for shift, low in ((44, 1 / 16), (43, 0.25), (42, 0.5), (46, 2.0 ** -16), (51, 2.0 ** -512)):
        assert S.warm_range_start(BITS_1, shift) == int(S.f64_bits([low])[0]), shift
    assert S.warm_range_start(0, 44) == S.NO_RANGE                                     # zero
    assert S.warm_range_start(int(S.f64_bits([2.0 ** -1020])[0]), 44) == S.NO_RANGE       # exponent field 3 <= 4 binades down
    assert S.warm_range_start(int(S.f64_bits([np.inf])[0]), 44) == S.NO_RANGE
    lo = S.warm_range_start(BITS_1, 44)
    keys = [lo - 1, lo, lo + (1 << 44) - 1, lo + (1 << 44), lo + (2046 << 44) - 1, lo + (2046 << 44)]
    assert list(S.warm_bin(keys, lo, 44)) == [0, 1, 1, 2, 2046, 2047]
    assert list(S.warm_bin(keys, S.NO_RANGE, 44)) == [0] * 6
    assert S.lower_median([3.0, 1.0, 2.0, 4.0]) == 2.0 and S.lower_median([5.0]) == 5.0 and S.lower_median([0.0, 7.0]) == 0.0


def _prefix_set(n_list, below, above):
    """``n_list`` keys sharing the top 32 bits of 2.7 -- hence also the bits above 42 that the compacted list is keyed on
    (``select_reference.LIST_SHIFT``) -- with ``below`` keys under and ``above`` keys over them, none of which shares even those."""
    base = (int(S.f64_bits([2.7])[0]) >> 31) << 31
    return _f([base + 5 * i for i in range(n_list)] + [BITS_1 + i for i in range(below)] + [int(S.f64_bits([8.0])[0]) + i for i in range(above)])


@pytest.mark.parametrize("n_list,branch", [(1024, "count"), (1026, "digits")])
def test_predict_exact_on_the_1024_limit(n_list, branch):
    for below, above in ((10, 10 + n_list % 2), (0, n_list), (n_list - 2, 0)):
        keys = _prefix_set(n_list, below, above)
        p = S.predict_exact(keys, keys.size)
        want = (keys.size - 1) // 2 - below
        assert (p["cnt"], p["rank"], p["branch"]) == (n_list, want, branch)
        assert p["key"] == S.lower_median(keys) == S.select_model(keys, keys.size // 2, keys.size // 2)


def _bin_set(lo, shift, bn, in_bin, below, above):
    return _f([lo + ((bn - 1) << shift) + 977 * i for i in range(in_bin)] + [lo + ((bn - 2) << shift) + i for i in range(below)]
              + [lo + (bn << shift) + i for i in range(above)])


def test_predict_warm_hits_misses_and_their_edges():
    lo = S.warm_range_start(BITS_1, 44)
    # a bin of exactly the capacity hits, one more key misses
    for in_bin, miss in ((256, None), (257, "full")):
        p = S.predict_warm(_bin_set(lo, 44, 1000, in_bin, 300, 300), lo, 44, 256)
        assert (p["bin"], p["in_bin"], p["miss"], p["hit"]) == (1000, in_bin, miss, miss is None)
        assert p["branch"] == (None if miss else "subbin")
    # the first and the last bin of the range hit, what lies outside misses
    inside = _f([lo + i for i in range(9)])
    assert S.predict_warm(inside, lo, 44, 256)["bin"] == 1 and S.predict_warm(inside, lo, 44, 256)["hit"]
    top = _f([lo + (2045 << 44) + i for i in range(9)])
    assert S.predict_warm(top, lo, 44, 256)["bin"] == 2046 and S.predict_warm(top, lo, 44, 256)["hit"]
    assert S.predict_warm(_f([lo - 1 - i for i in range(9)]), lo, 44, 256)["miss"] == "below"
    assert S.predict_warm(_f([lo + (2046 << 44) + i for i in range(9)]), lo, 44, 256)["miss"] == "above"
    assert S.predict_warm(inside, S.NO_RANGE, 44, 256)["miss"] == "no-range"
    assert S.predict_warm(inside, lo, 44, 256, force_miss=True)["miss"] == "forced"
    assert S.predict_warm(_bin_set(lo, 44, 1000, 257, 300, 300), lo, 44, 256, force_miss=True)["miss"] == "full"


def test_predict_warm_long_lists():
    lo = S.warm_range_start(BITS_1, 51)
    base = lo + (1023 << 51)
    for n_list, branch in ((1024, "subbin"), (1026, "long-first-digit")):
        keys = _f([base + (i << 40) + 3 * i for i in range(n_list)] + [lo + i for i in range(7)] + [base + (1 << 51) + i for i in range(7)])
        p = S.predict_warm(keys, lo, 51, 4096)
        assert (p["bin"], p["in_bin"], p["rank"], p["branch"]) == (1024, n_list, (keys.size - 1) // 2 - 7, branch)
        assert S.select_model(keys, keys.size // 2, keys.size // 2, dict(lo=lo, shift=51, list_cap=4096)) == S.lower_median(keys)
    # 1024 / 1026 keys inside ONE sub-bin of the first digit (2^40 bit patterns)
    for n_sub, branch in ((1024, "long-first-digit"), (1026, "long-radix")):
        keys = _f([base + (5 << 40) + 11 * i for i in range(n_sub)] + [base + i for i in range(40)] + [base + (9 << 40) + i for i in range(40)])
        p = S.predict_warm(keys, lo, 51, 4096)
        assert (p["in_bin"], p["sub_cnt"], p["branch"]) == (n_sub + 80, n_sub, branch)
        assert S.select_model(keys, keys.size // 2, keys.size // 2, dict(lo=lo, shift=51, list_cap=4096)) == S.lower_median(keys)


def test_sum_bound_is_the_depth_of_the_device_sum():
    assert S.sum_bound(1025, 5) == 29 * 2.0 ** -53 and S.sum_bound(4097, 17) == 29 * 2.0 ** -53 and S.sum_bound(1, 257) == 30 * 2.0 ** -53
    # an fp64 sum in the device's order (pairs, tree over 256, block partials in turn) stays within it
    rng = np.random.default_rng(0)
    k = np.exp2(rng.uniform(-20, 20, (4097, 2)))
    rows = np.zeros(17 * 256)
    rows[:4097] = k[:, 0] + k[:, 1]
    part = rows.reshape(17, 4, 64)
    for s in (32, 16, 8, 4, 2, 1):
        part = part[..., :s] + part[..., s:2 * s]
    part = ((part[:, 0, 0] + part[:, 1, 0]) + part[:, 2, 0]) + part[:, 3, 0]
    tot = float(np.add.reduce(part))
    assert abs(S.LD(tot) - S.exact_sum(k)) <= S.sum_bound(4097, 17) * S.exact_sum(k)


# ------------------------------------------------------------------------------------------------ the cases
def _fresh_cases():
    out = [(f"spread[{m}]", C.fresh(m), m) for m in C.KEY_COUNTS]
    out += [(f"{d}[{C.rows_1025(d)}]", C.fresh(C.rows_1025(d), d), C.rows_1025(d)) for d in C.DISTS_1025 if d != "spread"]
    return out + [("all-tied[512]", C.fresh(512, "all-tied"), 512)]


# case -> (shift, list capacity) -> what the second call's select does
CARRIED_BRANCH = {("tied-bin", 44, 256): "subbin", ("tied-bin", 46, 1200): "subbin", ("long-bin", 51, 4200): "long-first-digit",
                  ("long-ties", 51, 4200): "long-radix", ("m4097", 46, 8194): "subbin", ("m4097", 44, 256): "subbin",
                  ("leaving", 42, 256): "below", ("rising", 42, 256): "above", ("long-ties", 44, 256): "full", ("dup-bin", 44, 256): "subbin",
                  ("dup-bin", 46, 1200): "subbin"}
# the cases made for keys that differ inside the ranked set: a rank off by one either way is another value
DISTINCT = ("tied-bin", "long-bin", "long-ties", "m4097")


def _slot(c, m_max=None):
    k = C.device_order(C.oracle_keys(c), c.ii)
    return k if m_max is None else np.concatenate([k, np.zeros(2 * m_max - k.size)])


def _carried_slot(name, shift):
    c = C.carried(name)
    _k0, med0, k1, _ntr = C.oracle_call(c)
    return c, C.device_order(k1, c.ii), S.warm_range_start(int(S.f64_bits([med0])[0]), shift)


def test_fresh_cases_land_in_their_branch():
    seen = set()
    for name, c, m in _fresh_cases():
        k = C.oracle_keys(c)
        p = S.predict_exact(k, m)
        seen.add(p["branch"])
        if name in C.FRESH_BRANCH:
            assert (p["branch"], p["cnt"], p["rank"]) == C.FRESH_BRANCH[name], (name, p)
        else:
            assert p["branch"] == "count" and p["cnt"] < C.SHORT_LIST, (name, p)
        assert S.select_model(_slot(c), m, m) == S.lower_median(k), name
        assert S.select_model(_slot(c), m, m, items=S.SEL_ITEMS_BATCH) == S.lower_median(k), name
        print(f"{name}: {p['branch']}, list {p['cnt']}, rank {p['rank']}")
    assert seen == set(S.EXACT_BRANCHES)
    z = C.oracle_keys(C.fresh(1025, "zeros")).reshape(-1)
    assert 0 < (z == 0).sum() < z.size // 2 and S.lower_median(z) > 0.2
    w = np.unique(S.f64_bits(C.oracle_keys(C.fresh(1025, "wide"))) >> np.uint64(53)).size
    assert w >= 15, f"wide populates {w} digit-0 bins"


def test_stale_slot_and_batches():
    first, second = C.stale()
    old, new = _slot(first), _slot(second)
    slot = np.concatenate([new, old[new.size:]])
    assert S.select_model(slot, second.m, first.m) == S.lower_median(new) < C.STALE_OFFSET - 1 < S.lower_median(old)
    assert [c.m for c in C.ragged()] == [1025, 1, 256] and len(C.batch16()) == 16 and max(c.m for c in C.batch16()) == 257


def test_carried_cases_land_in_their_branch():
    seen = set()
    for (name, shift, cap), want in CARRIED_BRANCH.items():
        c, slot, lo = _carried_slot(name, shift)
        p = S.predict_warm(slot, lo, shift, cap)
        got = p["branch"] if p["hit"] else p["miss"]
        seen.add(got)
        print(f"{name} shift {shift} cap {cap}: {got}, bin {p['bin']}, list {p['in_bin']}, rank {p['rank']}, sub-bin {p['sub_cnt']}")
        assert got == want, (name, shift, cap, p)
        if p["hit"] and name in DISTINCT:
            assert p["sub_cnt"] > (1 if name in ("tied-bin", "long-ties") else 0), (name, shift, p)
            assert p["neighbours"] == int(p["sub_rank"] > 0) + int(p["sub_rank"] < p["sub_cnt"] - 1), (name, shift, p)
        if p["hit"]:
            assert S.select_model(slot, c.m, c.m, dict(lo=lo, shift=shift, list_cap=cap)) == S.lower_median(slot), name
    assert seen >= set(S.WARM_BRANCHES) | {"below", "above", "full"}
    # what the inline select's test needs of tied-bin: a bin of 9 .. 256 keys; what the misses need: the median leaves the range
    c, slot, lo = _carried_slot("tied-bin", 44)
    assert 9 <= S.predict_warm(slot, lo, 44, 256)["in_bin"] <= 256
    k0, med0, k1, _n = C.oracle_call(C.carried("leaving"))
    assert S.lower_median(k1) < 0.5 * med0
    k0, med0, k1, _n = C.oracle_call(C.carried("rising"))
    assert S.lower_median(k1) > 2.0 * med0
    # the exact copies tie bit for bit one call later too, and the median is one of them but not the first; the jittered copies differ
    c, slot, lo = _carried_slot("dup-bin", 44)
    p = S.predict_warm(slot, lo, 44, 256)
    assert np.unique(slot, return_counts=True)[1].max() == 40 and p["neighbours"] < 2 and (slot == S.lower_median(slot)).sum() == 40
    c, slot, lo = _carried_slot("tied-bin", 44)
    assert np.unique(slot, return_counts=True)[1].max() <= 2
    c, slot, lo = _carried_slot("long-ties", 51)
    p = S.predict_warm(slot, lo, 51, 4200)
    assert p["sub_cnt"] > 1024 and np.unique(slot, return_counts=True)[1].max() <= 4 and p["rank"] != p["sub_rank"], p


# ------------------------------------------------------------------------------------------------ planted faults
def _fresh_run(name, faults, items=S.SEL_ITEMS):
    for nm, c, m in _fresh_cases():
        if nm == name:
            return S.select_model(_slot(c), m, m, items=items, faults=faults), S.lower_median(C.oracle_keys(c))
    raise KeyError(name)


def _carried_run(name, shift, cap, faults):
    c, slot, lo = _carried_slot(name, shift)
    return S.select_model(slot, c.m, c.m, dict(lo=lo, shift=shift, list_cap=cap), faults=faults), S.lower_median(slot)


FAULTS = {
    "upper_median": lambda f: _fresh_run("spread[1025]", f),                # rank count // 2
    "count_limit_high": lambda f: _fresh_run("prefix-1026-last[1026]", f),  # a list of 1026 ranked by counting over the 1024 loaded entries
    "count_drops_last": lambda f: _fresh_run("prefix-1024-last[1025]", f),  # `<` for `<=`: the last entry of the list is not looked at
    "list_cap_short": lambda f: _fresh_run("all-tied[512]", f),             # `<` for `<=` at the list capacity: its last slot is not written
    "block_tail_dropped": lambda f: _fresh_run("spread[4097]", f),          # the last key pair of a full select block
    "tie_by_value": lambda f: _carried_run("dup-bin", 44, 256, f),          # equal keys all get the same rank
    "rank_not_rebased": lambda f: _carried_run("long-ties", 51, 4200, f),   # the rank inside the bin used again inside the sub-bin
    # warm_base from bin instead of bin - 1 (a short list does not see it: its sub-bin index is taken modulo 256 = one whole bin)
    "warm_base_bin": lambda f: _carried_run("long-bin", 51, 4200, f),
}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_planted_fault_is_caught(fault):
    got, ref = FAULTS[fault]((fault,))
    clean, ref2 = FAULTS[fault](())
    assert clean == ref == ref2, "the model without the fault is exact"
    print(f"{fault}: {got!r} where the lower median is {ref!r}")
    assert got != ref


def test_planted_fault_reading_the_whole_slot_is_caught_by_stale():
    first, second = C.stale()
    slot = np.concatenate([_slot(second), _slot(first)[2 * second.m:]])
    ref = S.lower_median(_slot(second))
    assert S.select_model(slot, second.m, first.m) == ref
    assert S.select_model(slot, second.m, first.m, faults=("reads_m_max",)) != ref


def test_block_fault_on_more_cases():
    """The dropped block tail on the other key counts beyond one select block.  (``list_cap_short`` is seen by all-tied[512] alone: on
    all-tied[1025] the key of the last slot lies above the median, and the digits over the rest still find the same key.)"""
    caught = [m for m in (1025, 4095, 4096, 4097) if _fresh_run(f"spread[{m}]", ("block_tail_dropped",))[0] != _fresh_run(f"spread[{m}]", ())[1]]
    assert 4097 in caught and len(caught) >= 2, caught
    got, ref = _fresh_run("spread[4097]", ("block_tail_dropped",), items=S.SEL_ITEMS_BATCH)
    assert got != ref, "the block tail at 32 keys per thread"
