"""Every path of the median select (``k_obs_residual`` in vinsat_amd/csrc/vba_obs.hip, ``k_select_pass`` / ``k_select_warm`` /
``k_select_finish`` in vba_select.hip, the bodies of vba_select_body.h that the accumulation's prologue calls) by the exact lower median
of the keys it selected from.

Each check has two parts.  The host PREDICTS the branch from what the device reports -- the keys (``|uv - debug("est")|`` of a call on
fresh states, ``debug_next()["keys"]`` of a carried one, with ``warm_lo``, ``shift`` and the histogram of the same fetch) through
tests/select_reference.py -- and asserts that it is the branch the case was made for: a case that drifts elsewhere fails, it does not
pass on another path.  Then ``c_obs`` must EQUAL ``lower_median`` of those keys: the select is exact, there is no tolerance.  The one
bar is ``sum_bound`` on the init residual of a landmark-only ``BA`` call, which is the sum of the keys over 2 m + 6 (n - 1) and nothing
else (no pose-chain term, no prior): a bound derived from the order of the device's sum, not a measurement.  tests/select_cases.py has
the windows, tests/test_select_reference_host.py the predictors on known key sets, the cases' conditions with the oracle's keys and
the planted faults.  Every case prints its predicted branch, list length and miss count.

Where each test lands:
  test_fresh[latency / bandwidth]   first call: k_obs_residual<true>, k_select_pass<1>, <2, compact> at 8 / 32 keys per thread, finish in the
                                    accumulation's prologue / in k_select_finish; branches ``count`` and ``digits``
  test_fresh_without_key_carry      ``set_key_carry(False)``: the second call is a fresh one too
  test_ragged_batch, test_default_mode_switch, test_stale_slot
                                    windows of 1025, 1 and 256 rows on one handle, both modes, each with the bits it has alone; 16 and
                                    200 windows on a handle that chooses its kernel set itself (latency / bandwidth); a slot whose longer first window left keys behind 2 m
  test_carried_exponent_histogram   ``set_warm_select(0)``: the trial left digit 0, k_select_pass<1> owns the resets
  test_inline_select_and_bucket_edge  latency default: the bucket of one warm bin ranked in the accumulation (``subbin``); a bucket of
                                    exactly in_bin keys hits, one of in_bin - 1 misses once (``full``) and repeats through
                                    k_clear_hist(2) and k_select_pass<0>; all three handles end in the same bits
  test_warm_kernel[wave / block]    k_select_warm<8> with the wave-aggregated append (``set_warm_select(3)``), k_select_warm<32> with the
                                    block reservation (bandwidth mode): ``subbin``, ``long-first-digit``, ``long-radix``, a list reserved
                                    from two blocks (4097 rows), a ragged batch
  test_real_misses                  the median leaves the range at shift 42: ``below`` and ``above``, alone and (bandwidth mode) beside a
                                    converged window that hits; ``forced`` on the ragged batch
  test_chained_twin                 ``run_schedule`` of the same two calls ends in the bits of the stepped handle
  test_every_reachable_branch_was_hit

Branches of ``select_finish_list`` that no accepted setting reaches (removing them is a follow-up):
  cnt <= kWarmCount in warm mode    needs warm_shift < 8 (the sub-bin branch in front of it takes every list of <= 1024 keys otherwise);
                                    ``vba_set_warm_shift`` accepts 42 .. 51
  remaining <= 11                   the same: remaining = warm_shift >= 42
  lo == ~0 (``no-range``)           a carried median that is zero or denormal; the weights of the call that produced it are not finite,
                                    and no case was found that gets there otherwise
The overflow fallback (cnt > 2 m_max) is not among them: the handles of this module hold all their keys, but a sharded handle selects
among the gathered keys of all ranks with a list sized for its own slice.  tests/test_gpu_sharded_stages.py runs it, short and long.
"""
import numpy as np
import pytest

import select_cases as C
import select_reference as S

pytestmark = pytest.mark.gpu

SEEN = set()
_ALONE = {}
_CARRIED = {}
FRESH = [(f"spread[{m}]", m, "spread") for m in C.KEY_COUNTS] + \
        [(f"{d}[{C.rows_1025(d)}]", C.rows_1025(d), d) for d in C.DISTS_1025 if d != "spread"] + [("all-tied[512]", 512, "all-tied")]
MODES = {"latency": 1, "bandwidth": 0}


def engine(n_max, m_max, windows=1, mode=1, carry=True, warm=None, shift=None, cap=None):
    from vinsat_amd.engine import BAEngine
    e = BAEngine(n_max, m_max, windows=windows, mode=mode)
    if not carry:
        e.set_key_carry(False)
    if warm is not None:
        e.set_warm_select(warm)
    if shift is not None:
        e.set_warm_shift(shift)
    if cap is not None:
        e.set_bucket_cap(cap)
    return e


def upload(e, c, k=0):
    e.upload_observations(c.xyz, c.uv, c.conf, c.ii, c.n, window=k)
    e.upload_window(c.K, c.cumrot, c.t, window=k)
    e.set_states(c.states, C.LAM, window=k)


def fresh_keys(e, c, k=0):
    return np.abs(c.uv - e.debug("est", window=k))


def check_fresh(e, c, k, where, m_max):
    """One window after a call on fresh states: the predicted branch -- the one of ``select_cases.FRESH_BRANCH`` with its list length
    and rank, a list of different keys; for every other case ``count`` on a short list -- the exact median, the sum.  Returns (keys, c_obs)."""
    want = C.FRESH_BRANCH.get(c.name)
    keys = fresh_keys(e, c, k)
    sc = e.debug("scalars", window=k)
    p = S.predict_exact(keys, m_max)
    SEEN.add(p["branch"])
    print(f"{where}: {p['branch']}, list {p['cnt']}, rank {p['rank']}, misses {e.warm_select_misses()}")
    if want is not None:
        assert (p["branch"], p["cnt"], p["rank"]) == want, f"{where}: made for {want}, the device's keys give {p}"
        assert p["neighbours"] == (2 if 0 < p["rank"] < p["cnt"] - 1 else 1), f"{where}: the wanted key's neighbours in the list equal it: {p}"
    else:
        assert p["branch"] == "count" and p["cnt"] < C.SHORT_LIST, f"{where}: made for a short list, the device's keys give {p}"
    assert sc[0] == S.lower_median(keys), f"{where}: c_obs {sc[0]!r}, the lower median of its keys is {S.lower_median(keys)!r}"
    ref = S.exact_sum(keys) / S.LD(2 * c.m + 6 * (c.n - 1))
    bound = S.sum_bound(c.m, -(-m_max // 256))
    print(f"{where}: init residual off by {float(abs(S.LD(sc[2]) - ref) / ref) * 2.0 ** 53:.2f} x 2^-53 (bound {bound * 2.0 ** 53:.0f})")
    assert abs(S.LD(sc[2]) - ref) <= bound * ref, f"{where}: init residual {sc[2]!r}, the sum of the keys gives {float(ref)!r}"
    return keys, sc[0]


def alone(c, mode):
    """(keys, c_obs) of the first call on ``c`` on a handle of its own."""
    key = (c.name, mode)
    if key not in _ALONE:
        e = engine(c.n, c.m, mode=mode)
        upload(e, c)
        e.step(C.IT, True)
        _ALONE[key] = check_fresh(e, c, 0, f"{c.name} {mode}", c.m)
        e.close()
    return _ALONE[key]


# ------------------------------------------------------------------------------------------------ fresh states
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name,m,dist", FRESH, ids=[f[0] for f in FRESH])
def test_fresh(name, m, dist, mode):
    c = C.fresh(m, dist)
    assert c.name == name
    alone(c, MODES[mode])


def test_fresh_without_key_carry():
    for mode in (1, 0):
        c = C.fresh(1025, "spread")
        e = engine(c.n, c.m, mode=mode, carry=False)
        upload(e, c)
        e.step(C.IT, True)
        e.step(C.IT, True)
        keys, _c = check_fresh(e, c, 0, f"{c.name} second call, no carry, mode {mode}", c.m)
        assert not np.array_equal(keys, alone(c, mode)[0]), "the second call ran at the states of the first"
        e.close()


def batch(cs, mode, m_max, where):
    e = engine(16, m_max, windows=len(cs), mode=mode)
    for k, c in enumerate(cs):
        upload(e, c, k)
    e.step(C.IT, True)
    lat = e.mode()[0]
    for k, c in enumerate(cs):
        keys, med = check_fresh(e, c, k, f"{where} w={k} {c.name}", m_max)
        a_keys, a_med = alone(c, lat)
        assert np.array_equal(keys, a_keys) and med == a_med, f"{where} w={k}: other bits than the window alone"
    e.close()
    return lat


@pytest.mark.parametrize("mode", list(MODES))
def test_ragged_batch(mode):
    batch(C.ragged(), MODES[mode], 1025, f"ragged {mode}")


def test_default_mode_switch():
    """A handle that chooses its kernel set itself (``mode=-1``).  The switch follows the rows per window as well as the window count
    (``default_latency_mode``: up to 38 (50000 / m_max)^0.7 windows, 192 at the most, keep the latency set): 16 windows of 257 rows stay
    with the latency-mode kernels, 200 take the bandwidth-mode ones.  Every window against the window alone on the same kernel set."""
    assert batch(C.batch16(), -1, 257, "16 windows") == 1
    assert batch(C.batch_over_the_switch(), -1, 257, "200 windows") == 0


@pytest.mark.parametrize("mode", list(MODES))
def test_stale_slot(mode):
    first, second = C.stale()
    e = engine(16, first.m, mode=MODES[mode])
    upload(e, first)
    e.step(C.IT, True)
    check_fresh(e, first, 0, f"stale first {mode}", first.m)
    upload(e, second)
    e.step(C.IT, True)
    keys, med = check_fresh(e, second, 0, f"stale second {mode}", first.m)
    assert med < C.STALE_OFFSET - 1 and med == alone(second, MODES[mode])[1]
    e.close()


# ------------------------------------------------------------------------------------------------ carried keys
def carried(names, mode=1, warm=None, shift=None, cap=None, chained=False, n_max=16):
    """Two landmark-only calls on the windows ``names`` of one handle; per window what the first call left, the prediction for the
    second call's select from it, and the second call's median and states.  Cached."""
    key = (tuple(names), mode, warm, shift, cap, chained)
    if key in _CARRIED:
        return _CARRIED[key]
    cs = [C.carried(n) if n in C.CARRIED else C.fresh(*n) for n in names]
    m_max = max(c.m for c in cs)
    e = engine(n_max, m_max, windows=len(cs), mode=mode, warm=warm, shift=shift, cap=cap)
    for k, c in enumerate(cs):
        upload(e, c, k)
    out = dict(windows=[], m_max=m_max)
    if chained:
        e.run_schedule([C.IT, C.IT], [True, True])
    else:
        e.step(C.IT, True)
        nxt = [e.debug_next(k) for k in range(len(cs))]
        e.step(C.IT, True)
    out["misses"] = e.warm_select_misses()
    inline = e.mode()[0] == 1 and warm in (None, 1)
    for k, c in enumerate(cs):
        w = dict(states=e.get_states(window=k), c_obs=e.debug("scalars", window=k)[0], case=c)
        if not chained:
            nx = nxt[k]
            w["next"] = nx
            keys = nx["keys"]
            assert np.array_equal(keys, fresh_keys(e, c, k)), f"{c.name}: the carried keys are not |uv - est| at the second call's states"
            where = f"{'+'.join(str(n) for n in names)} w={k} mode {mode} warm {warm} shift {shift} cap {cap}"
            if nx["kind"] == 2:
                cap_k = nx["cap"] if inline else 2 * m_max
                p = S.predict_warm(C.device_order(keys, c.ii), nx["warm_lo"], nx["shift"], cap_k, force_miss=warm == 2)
                assert int(nx["hist"][p["bin"]]) == p["in_bin"], f"{where}: the histogram's bin {p['bin']} disagrees with the keys"
                w["path"] = p["branch"] if p["hit"] else p["miss"]
                print(f"{where}: {w['path']}, bin {p['bin']}, list {p['in_bin']}, rank {p['rank']}, sub-bin {p['sub_cnt']}, misses {out['misses']}")
            else:
                p = S.predict_exact(keys, m_max)
                w["path"] = "carried-" + p["branch"]
                print(f"{where}: exponent histogram, {p['branch']}, list {p['cnt']}, rank {p['rank']}, misses {out['misses']}")
            if nx["kind"] == 2 and p["hit"] and c.name in DISTINCT:
                assert p["sub_cnt"] > (1 if c.name in ("tied-bin", "long-ties") else 0) and p["neighbours"] == int(p["sub_rank"] > 0) + int(p["sub_rank"] < p["sub_cnt"] - 1), \
                    f"{where}: the set that is ranked last holds equal keys beside the wanted one: {p}"
            w["pred"] = p
            SEEN.add(w["path"])
            assert w["c_obs"] == S.lower_median(keys), f"{where}: c_obs {w['c_obs']!r}, the lower median of the carried keys is {S.lower_median(keys)!r}"
        out["windows"].append(w)
    e.close()
    _CARRIED[key] = out
    return out


# the carried cases made for keys that differ inside the set that is ranked last: a rank off by one either way is another value
DISTINCT = ("tied-bin", "long-bin", "long-ties", "m4097")


def same_end(a, b, what):
    for wa, wb in zip(a["windows"], b["windows"]):
        sa, sb = wa["states"], wb["states"]
        assert np.array_equal(sa[0], sb[0]) and sa[1] == sb[1] and sa[3:] == sb[3:] and wa["c_obs"] == wb["c_obs"], what


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ["tied-bin", "m4097"])
def test_carried_exponent_histogram(name, mode):
    r = carried([name], mode=MODES[mode], warm=0)
    assert r["windows"][0]["path"] == "carried-count" and r["misses"] == 0


def test_inline_select_and_bucket_edge():
    twin = carried(["tied-bin"])
    w = twin["windows"][0]
    in_bin = w["pred"]["in_bin"]
    assert w["path"] == "subbin" and twin["misses"] == 0 and w["next"]["cap"] == 256
    assert 9 <= in_bin <= 256, in_bin
    fits = carried(["tied-bin"], cap=in_bin)
    assert fits["windows"][0]["path"] == "subbin" and fits["misses"] == 0
    tight = carried(["tied-bin"], cap=in_bin - 1)
    assert tight["windows"][0]["path"] == "full" and tight["misses"] == 1
    same_end(fits, twin, "a bucket of exactly in_bin keys")
    same_end(tight, twin, "the exact repeat behind a full bucket")
    dup = carried(["dup-bin"])        # the median is one of 40 equal keys: ties broken by position
    assert dup["windows"][0]["path"] == "subbin" and dup["misses"] == 0 and dup["windows"][0]["pred"]["neighbours"] < 2


WARM_KERNEL = {"wave": dict(mode=1, warm=3), "block": dict(mode=0)}


@pytest.mark.parametrize("form", list(WARM_KERNEL))
def test_warm_kernel(form):
    kw = WARM_KERNEL[form]
    for name, shift, want in (("tied-bin", None, "subbin"), ("dup-bin", None, "subbin"), ("long-bin", 51, "long-first-digit"),
                              ("long-ties", 51, "long-radix")):
        r = carried([name], shift=shift, **kw)
        assert r["windows"][0]["path"] == want and r["misses"] == 0, (name, r["windows"][0]["path"], r["misses"])
        assert r["windows"][0]["next"]["shift"] == (shift or (44 if kw["mode"] == 1 else 46))
    if form == "block":
        r = carried(["m4097"], **kw)        # 8194 keys: the second block of k_select_warm<32> holds two
        assert r["windows"][0]["path"] == "subbin" and r["misses"] == 0
        r = carried(["tied-bin", (1, "spread"), "long-bin"], **kw)
        assert [w["path"] for w in r["windows"]] == ["subbin"] * 3 and r["misses"] == 0


def test_real_misses():
    for name, want in (("leaving", "below"), ("rising", "above")):
        n_max = C.carried(name).n
        r = carried([name], shift=42, n_max=n_max)
        assert r["windows"][0]["path"] == want and r["misses"] == 1, (name, r["windows"][0]["path"], r["misses"])
        r = carried([name], mode=0, shift=42, n_max=n_max)
        assert r["windows"][0]["path"] == want and r["misses"] == 1
    # beside a window that hits: one miss counted for the call, both medians exact
    r = carried(["rising", "long-bin"], mode=0, shift=42)
    assert [w["path"] for w in r["windows"]] == ["above", "subbin"] and r["misses"] == 1, [w["path"] for w in r["windows"]]
    r = carried(["leaving", "long-bin"], mode=0, shift=42)
    assert [w["path"] for w in r["windows"]] == ["below", "subbin"] and r["misses"] == 1, [w["path"] for w in r["windows"]]
    # every carried call forced to miss
    for mode in (1, 0):
        r = carried(["tied-bin", (1, "spread"), "long-bin"], mode=mode, warm=2)
        assert [w["path"] for w in r["windows"]] == ["forced"] * 3 and r["misses"] == 1


@pytest.mark.parametrize("kw", [dict(), dict(warm=0), dict(warm=3), dict(mode=0), dict(shift=42, names=["rising"])],
                         ids=["inline", "exponent", "wave", "block", "miss"])
def test_chained_twin(kw):
    kw = dict(kw)
    names = kw.pop("names", ["tied-bin"])
    same_end(carried(names, chained=True, **kw), carried(names, **kw), f"run_schedule against two steps {kw}")


def test_every_reachable_branch_was_hit():
    alone(C.fresh(1025, "prefix-1024-mid"), 1)
    alone(C.fresh(1025, "prefix-1026-mid"), 1)
    carried(["tied-bin"])
    carried(["tied-bin"], cap=carried(["tied-bin"])["windows"][0]["pred"]["in_bin"] - 1)
    carried(["long-bin"], mode=0, shift=51)
    carried(["long-ties"], mode=0, shift=51)
    carried(["leaving"], shift=42, n_max=8)
    carried(["rising"], shift=42)
    carried(["tied-bin", (1, "spread"), "long-bin"], mode=1, warm=2)
    want = set(S.EXACT_BRANCHES) | set(S.WARM_BRANCHES) | (set(S.MISSES) - {"no-range"})
    print("branches hit:", sorted(SEEN))
    assert want <= SEEN, f"not reached: {sorted(want - SEEN)}"
