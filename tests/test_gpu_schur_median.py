"""``vba_schur_median`` / ``schur.median`` on the GPU: the exact radix select of ``vba_schur_reweight`` on caller keys, bit for bit
``numpy.sort(keys)[(count - 1) // 2]``.

Counts sit on every boundary of the select as csrc/vba_schur_robust.h shapes it (keys of a thread, of a workgroup's tile, of a
launch, the switch from the one-workgroup path), each at -1, 0 and +1; the key sets are those a projection cannot produce on
demand: ties, zeros, denormals, infinities, keys that differ in their last digit only.  Every test needs the entry point and fails
where it does not exist.
"""
import ctypes

import numpy as np
import pytest

import schur_robust_reference as RR

pytestmark = pytest.mark.gpu
K = RR.select_constants()
TILE = K["kSelThreads"] * K["kSelKeysPerThread"]
BOUNDARIES = (K["kSelKeysPerThread"], 2 * K["kSelThreads"], TILE, K["kSelSmallMax"], K["kSelSmallMax"] + TILE, K["kSelMaxBlocks"] * TILE)
COUNTS = (1, 2, 3, 4) + tuple(b + o for b in BOUNDARIES for o in (-1, 0, 1)) + (100_001,)
SET_COUNTS = (4, TILE + 1, K["kSelSmallMax"], K["kSelSmallMax"] + 1, 3 * TILE + 5, 100_001)


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def _check(keys, label):
    from vinsat_amd import schur
    keys = np.ascontiguousarray(keys, dtype=np.float64)
    want = np.sort(keys)[(keys.size - 1) // 2]
    got = np.float64(schur.median(keys))
    again = np.float64(schur.median(keys))
    assert _bits(got) == _bits(want), f"{label}: count {keys.size} got {got!r} want {want!r}"
    assert _bits(again) == _bits(got)


def _key_set(kind, count):
    rng = np.random.default_rng(count + 17)
    if kind == "lognormal":
        return rng.lognormal(0.0, 2.0, count)
    if kind == "all_equal":
        return np.full(count, 0.7312)
    if kind == "tie_run":           # a run of equal keys around the median, longer than a workgroup's tile where the count allows
        run = min(count, max(count // 3, TILE + 7))
        lo = (count - run) // 2
        keys = np.concatenate([rng.uniform(0.0, 1.0, lo), np.full(run, 1.5), rng.uniform(2.0, 3.0, count - run - lo)])
        return rng.permutation(keys)
    if kind == "half_zero":         # the last +0 is the median of an even count
        keys = rng.lognormal(0.0, 1.0, count)
        keys[rng.permutation(count)[: max(count // 2, 1)]] = 0.0
        return keys
    if kind == "denormals":
        return rng.integers(1, 1 << 52, count, dtype=np.uint64).view(np.float64)
    if kind == "inf_tail_above":    # 40 % +inf: a finite median
        keys = rng.lognormal(0.0, 1.0, count)
        keys[rng.permutation(count)[: (2 * count) // 5]] = np.inf
        return keys
    if kind == "inf_tail_across":   # 60 % +inf: the median is +inf
        keys = rng.lognormal(0.0, 1.0, count)
        keys[rng.permutation(count)[: (3 * count) // 5 + 1]] = np.inf
        return keys
    if kind == "last_digit":        # equal in every digit of the select but the last
        return (np.float64(3.25).view(np.uint64) + rng.integers(0, 1 << K["kSelDigitBits"], count, dtype=np.uint64)).view(np.float64)
    raise KeyError(kind)


KINDS = ("lognormal", "all_equal", "tie_run", "half_zero", "denormals", "inf_tail_above", "inf_tail_across", "last_digit")


def test_counts_cover_both_paths():
    assert min(COUNTS) == 1 and any(c <= K["kSelSmallMax"] for c in COUNTS) and any(c > K["kSelMaxBlocks"] * TILE for c in COUNTS)


@pytest.mark.parametrize("count", COUNTS)
def test_lower_median_at_every_boundary(count):
    _check(_key_set("lognormal", count), "lognormal")
    _check(_key_set("last_digit", count), "last_digit")


@pytest.mark.parametrize("kind", KINDS)
def test_key_sets(kind):
    for count in SET_COUNTS:
        keys = _key_set(kind, count)
        assert keys.size == count and not np.isnan(keys).any() and not np.signbit(keys).any()
        _check(keys, kind)


def test_the_sets_are_what_they_claim():
    c = SET_COUNTS[-1]
    tie = _key_set("tie_run", c)
    assert (tie == 1.5).sum() > TILE and np.sort(tie)[(c - 1) // 2] == 1.5
    assert np.sort(_key_set("half_zero", c - 1))[(c - 2) // 2] == 0.0 and np.sort(_key_set("half_zero", c - 1))[(c - 2) // 2 + 1] > 0.0
    assert np.all(_key_set("denormals", c) < np.finfo(np.float64).tiny)
    assert np.isinf(np.sort(_key_set("inf_tail_across", c))[(c - 1) // 2]) and np.isfinite(np.sort(_key_set("inf_tail_above", c))[(c - 1) // 2])
    d = _key_set("last_digit", c).view(np.uint64)
    assert np.unique(d >> np.uint64(K["kSelDigitBits"])).size == 1 and np.unique(d).size > 1


def test_bad_keys_and_counts_are_refused():
    from vinsat_amd import _lib, schur
    lib = _lib.load()
    good = np.array([1.0, 2.0, 3.0])
    for bad in (np.array([1.0, np.nan, 3.0]), np.array([1.0, -2.0, 3.0]), np.array([1.0, -0.0, 3.0])):
        out = ctypes.c_double(-1.0)
        assert lib.vba_schur_median(0, bad.ctypes.data_as(_lib.PD), bad.size, ctypes.byref(out)) == 1      # VBA_EINVAL
        with pytest.raises(_lib.VbaError):
            schur.median(bad)
    for count in (0, -1):
        out = ctypes.c_double(-1.0)
        assert lib.vba_schur_median(0, good.ctypes.data_as(_lib.PD), count, ctypes.byref(out)) == 1
    with pytest.raises(_lib.VbaError):
        schur.median(np.empty(0))
    assert schur.median(good) == 2.0
