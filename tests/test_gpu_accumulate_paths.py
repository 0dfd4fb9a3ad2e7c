"""Every form of k_obs_accumulate (vinsat_amd/csrc/vba_accumulate.hip) by its per-pose sums, depth-clamped rows included.

One BA call per case at the case's states (tests/accumulate_cases.py), then ``vba_debug_fetch``: the per-pose ``H``, ``b`` the kernel
left, and ``est``, ``weight``, ``Jg`` of the rows.  Layer A judges the sums against the longdouble sums of those very rows, layer B the
rows against the longdouble rows (tests/accumulate_reference.py); a figure passes at K x 2^-53 with K = max(16, 4 x the fp64 NumPy
oracle's figure on the same case).  tests/test_accumulate_reference_host.py holds the oracle's table and shows that a dropped or
doubled row, a leaking pair, a missing lane, a wrong ``live`` flag and a relative 1e-9 in a small pose all fail these bars.

Where each test lands (launch_obs_accumulate):

  test_latency_set          mode 1, one window: k_obs_accumulate<G, PAIR (4, 8), false>, CAM for G <= 16, per-row J for 32 / 64; first
                            ``vba_step`` behind ``vba_set_states``: the exact select inside the kernel; for clamped(G) a second ``vba_step``
                            behind the accepted one: the inline select from the keys that trial carried (no miss allowed; a twin
                            handle with forced misses shows that the warm select was attempted on exactly that call)
  test_bandwidth_set        mode 0, 16 ragged windows: lanes 8, 16 -> the BATCH instantiation with one group per block; 4, 32, 64 -> the
                            plain kernel behind k_select_finish (median_ready)
  test_group_walk           mode 0, 1024 windows of up to 130 poses: BATCH with groups = 4 (gstride, pf_beg / pf_end), 2 and 3 blocks per window
  test_fp32_jacobian        F32 instantiations: lanes 4, 64 (latency set) and BATCH 8
  test_rows_do_not_depend_on_lanes   est and weight bit-equal over the five lane counts, both kernel sets
  test_whole_call           clamped(8) through random_windows.SCHEDULE against the oracle call by call: k_trial's projection meets
                            80 .. 170 clamped rows in every trial

Measured on the MI355X: the largest figure per path and layer in units of 2^-53, beside it in brackets the oracle's figure on the
case that gave it (the bar is max(16, 4 x the bracket)).  Layer A: H (tt, tr, rr together), b (t, r); layer B: est, J_t, J_r, w.

  path                         H            b            est          J_t          J_r          w
  latency first call   G=4     2.10 (3.87)  1.95 (4.61)  4.79 (3.47)  5.76 (4.39)  6.61 (5.24)  3.13 (2.95)
                       G=8     2.16 (3.12)  2.37 (2.57)  5.38 (4.06)  5.92 (4.86)  8.04 (5.46)  3.83 (2.88)
                       G=16    1.68 (2.66)  1.79 (4.52)  5.43 (4.06)  5.92 (4.86)  7.68 (7.11)  4.18 (2.70)
                       G=32    1.59 (2.82)  1.47 (3.40)  5.70 (4.06)  5.95 (4.68)  7.47 (6.38)  4.42 (3.66)
                       G=64    1.37 (4.02)  1.88 (6.92)  5.74 (4.18)  5.95 (4.92)  8.43 (6.70)  3.54 (3.66)
  latency chained call G=4     1.98 (3.40)  1.63 (3.27)
  (inline select)      G=8     2.15 (2.37)  2.04 (3.42)
                       G=16    1.97 (3.38)  2.20 (4.81)
                       G=32    1.48 (4.40)  1.39 (4.50)
                       G=64    1.29 (3.82)  1.46 (4.67)
  bandwidth, 16 windows G=4    3.09 (1.79)  2.52 (2.66)  4.79 (3.47)  5.76 (4.39)  6.61 (5.24)  3.61 (3.66)
                       G=8     2.49 (2.57)  2.53 (5.83)  5.38 (4.06)  5.92 (4.86)  8.04 (5.46)  4.42 (4.06)
                       G=16    2.08 (2.49)  1.93 (4.35)  5.43 (4.06)  5.92 (4.86)  7.68 (7.11)  4.18 (2.70)
                       G=32    1.67 (2.09)  1.83 (2.72)  5.70 (4.06)  5.95 (4.68)  7.47 (6.38)  4.64 (3.85)
                       G=64    1.62 (3.96)  1.96 (4.57)  5.74 (4.18)  5.95 (4.92)  8.43 (6.70)  3.76 (3.98)
  group walk, 1024     G=8     2.71 (0.95)  2.29 (1.12)
                       G=16    2.71 (0.95)  1.77 (1.12)
  fp32 terms           G=4     1.81 (2.69)  1.60 (3.53)
                       G=64    1.78 (4.34)  1.49 (5.83)
                       BATCH 8 2.01 (3.07)  2.75 (2.82)

Nothing comes near a bar (16 at the least): the sums of every path stand 1.3 .. 3.1 units from the longdouble sums of their own rows
-- below NumPy's sequential ``add.at`` in most places, as a tree of partial sums should -- and the rows 3 .. 8.5 units from the
longdouble rows, one to two units above NumPy (the refined reciprocal and the contracted products of project_jacobian).  Every
repeat of the walk was bit-equal to its first occurrence, no pose slot behind a window's last pose was written, est and weight had
the same bits at every lane count.  The chained rows are second ``vba_step`` calls on the inline-select path: no miss on the handle
under test, exactly one on its forced-miss twin at every lane count, and the twin's exact repeat left the same bits.  The whole call on clamped(8) agreed with the oracle in
trial counts and damping in all 6 calls of both kernel sets; positions within 8.2e-12, attitude within 8.3e-7 rad (call 0, landmark
only; 1.5e-13 rad in the full phase), the last trial residual within 3.0e-10 relative (bar 1e-9).  No defect was found in
vba_accumulate.hip or vba_math.h.
"""
import numpy as np
import pytest

import accumulate_cases as C
import accumulate_reference as A
import random_windows
from conftest import rel_err
from oracle import ba_oracle as O

pytestmark = pytest.mark.gpu

LANES = (4, 8, 16, 32, 64)
IT, IT2 = C.IT, 14
_LEVELS = {}


def levels(case, it=IT, states=None, tag=""):
    key = (case.name, case.n, case.m, it, tag)
    if key not in _LEVELS:
        _LEVELS[key] = A.oracle_levels(case.states if states is None else states, case.xyz, case.K, case.uv, case.ii, case.conf, it, case.n)
    return _LEVELS[key]


def engine(n_max, m_max, windows=1, mode=1, lanes=None, f32=False):
    from vinsat_amd.engine import BAEngine
    e = BAEngine(n_max, m_max, windows=windows, mode=mode)
    if lanes is not None:
        e.set_accumulate_lanes(lanes)
    if f32:
        e.set_jacobian_f32(True)
    return e


def upload(e, case, k=0, states=True):
    e.upload_observations(case.xyz, case.uv, case.conf, case.ii, case.n, window=k)
    e.upload_window(case.K, case.cumrot, case.t, window=k)
    if states:
        e.set_states(case.states, 1e-4, window=k)


def fetch(e, k=0, rows=True):
    d = {w: e.debug(w, window=k) for w in (("H", "b", "scalars", "est", "weight", "Jg") if rows else ("H", "b", "scalars"))}
    d["w"] = d.pop("weight", None)
    return d


def check(case, d, lv, where, layers="AB", states=None, it=IT):
    """[] or what is out of bounds; prints the figures of this fetch."""
    bad = []
    if not (d["scalars"][3] == d["scalars"][3] and np.isfinite(d["H"]).all()):
        bad.append(f"{where}: non-finite sums or trial residual")
    a = A.layer_a(d["H"], d["b"], d["est"], d["w"], d["Jg"], case.uv, case.ii, case.n)
    b = None
    if "B" in layers:
        b = A.layer_b(case.states if states is None else states, case.xyz, case.K, case.uv, case.ii, case.conf, it, d["est"], d["Jg"], d["w"],
                      d["scalars"][0], d["scalars"][1], lv.rows)
    v = A.judge(lv, a, b)
    print(f"FIGURES {where}: " + " ".join(f"{k}={v.units[k]:.2f}/{lv.units[k]:.2f}" for k in v.units))
    bad += [f"{where}: {f}" for f in v.failures]
    empty = case.counts == 0
    if empty.any() and not (np.all(d["H"][empty] == 0.0) and np.all(d["b"][empty] == 0.0)):
        bad.append(f"{where}: a pose without rows does not have exact zeros")
    return bad


def truncated(case, n):
    """The first n poses of a case with their rows."""
    if n == case.n:
        return case
    keep = case.ii < n
    ex = {k: (v[keep] if isinstance(v, np.ndarray) and v.shape[:1] == (case.m,) else v) for k, v in case.extras.items()}
    return C.Case(f"{case.name}[:{n}]", case.states[:n].copy(), case.xyz[keep], case.uv[keep], case.conf[keep], case.ii[keep], case.K[:n],
                  case.cumrot[:n], case.t[:n], case.counts[:n], case.moved[keep], ex)


# ------------------------------------------------------------------------------------------------ latency set
def exact_median(case, est):
    a = np.abs(case.uv - est).reshape(-1)
    return np.sort(a)[(a.size - 1) // 2]


@pytest.mark.parametrize("G", LANES)
def test_latency_set(G):
    """First call: ``vba_set_states`` drops whatever was carried, so the kernel finishes the exact select itself (select_finish).
    ``vba_step`` has its trial leave the next call's |r| keys in the bin buckets, so the second ``step`` of clamped(G) enters
    k_obs_accumulate with sel_inline = 1 (enqueue_front: carry == 2, bin buckets allocated, inline select on).  That this is the
    path that ran is shown three ways: the handle has bin buckets (``set_bucket_cap`` raises on one that has none); a twin handle
    with every warm select forced to miss (``set_warm_select(2)``) counts exactly one miss, on that second call -- a warm select was
    attempted there and nowhere else -- while the handle under test counts none; and the twin, which repeats the front with the exact
    digits, leaves the same bits, so the median the inline select ranked out of its bucket is the exact one."""
    bad = []
    for case in (C.edges(G, 0), C.edges(G, 1), C.clamped(G)):
        chained = case.name.startswith("clamped")
        second = {}
        for warm in ((1, 2) if chained else (1,)):
            e = engine(case.n, case.m, mode=1, lanes=G)         # m_max == m
            e.set_warm_select(warm)
            e.set_bucket_cap(0)                                 # (the allocated capacity; VbaError on a handle without bin buckets)
            upload(e, case)
            e.step(IT, False)
            out, _, _, _, flags = e.get_states()
            assert flags == 0 and e.warm_select_misses() == 0
            d = fetch(e)
            assert d["scalars"][0] == exact_median(case, d["est"])
            if warm == 1:
                bad += check(case, d, levels(case), f"latency G={G} {case.name} first call")
            if chained:
                assert d["scalars"][3] < d["scalars"][2], "the first call did not accept its trial: nothing is carried"
                e.step(IT2, False)
                assert e.warm_select_misses() == (0 if warm == 1 else 1), (warm, e.warm_select_misses())
                assert e.get_states()[4] == 0
                d2 = fetch(e)
                assert d2["scalars"][0] == exact_median(case, d2["est"])
                second[warm] = d2
                if warm == 1:
                    lv2 = levels(case, IT2, states=out, tag=f"behind G={G}")
                    bad += check(case, d2, lv2, f"latency G={G} {case.name} chained call", layers="A", states=out, it=IT2)
            e.close()
        if chained:
            a, b = second[1], second[2]
            for k in ("H", "b", "est", "w"):
                assert np.array_equal(a[k], b[k]), f"G={G}: {k} of the inline select differs from the exact repeat"
            assert np.array_equal(a["scalars"][:4], b["scalars"][:4])
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ bandwidth set
RAGGED = (70, 70, 70, 69, 37, 36, 64, 5, 2, 66, 33, 14, 70, 27, 3, 65)


@pytest.mark.parametrize("G", LANES)
def test_bandwidth_set(G):
    base = (C.edges(G, 0), C.edges(G, 1), C.clamped(G))
    wins = [truncated(base[k % 3], n) for k, n in enumerate(RAGGED)]
    e = engine(70, max(w.m for w in wins), windows=len(wins), mode=0, lanes=G)
    for k, w in enumerate(wins):
        upload(e, w, k)
    e.step(IT, False)
    bad = []
    for k, w in enumerate(wins):
        assert e.get_states(window=k)[4] == 0
        bad += check(w, fetch(e, k), levels(w), f"bandwidth G={G} w={k} {w.name}")
    e.close()
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ the group walk
ULP4 = 4.01 * 2.0 ** -53


@pytest.mark.parametrize("G", [8, 16])
def test_group_walk(G):
    """1024 windows, groups = 4.  The 8 distinct windows by layer A, every repeat bit-equal to its first occurrence, and the pose slots
    behind a window's last pose untouched.  The last is seen like this: two calls on 1024 copies of the 130-pose window leave known
    sums in all 130 slots of both call parities; after the call on the ragged windows the 130-pose rows are uploaded again (no call),
    which makes the fetch hand out all 130 slots.  A fetched H is H_raw / w_max, so slot i >= n[w] must hold H_1[i] w_max_1 / w_max_2
    for one of the two earlier calls: four roundings, |H_3 w_max_2 - H_1 w_max_1| <= 4.01 x 2^-53 |H_1 w_max_1| entry by entry."""
    wins = C.walk()
    W, N = C.WALK_WINDOWS, C.WALK_N_MAX
    assert C.walk_groups(G)[0] == 4
    e = engine(N, max(w.m for w in wins), windows=W, mode=0, lanes=G)
    full = wins[0]
    for k in range(W):
        upload(e, full, k)
    before = []
    for it in (IT, IT2):
        e.step(it, False)
        Hs = np.stack([e.debug("H", window=k) for k in range(W)])
        wm = np.array([e.debug("scalars", window=k)[1] for k in range(W)])
        assert np.all(Hs == Hs[0]) and np.all(wm == wm[0]), "equal windows, different sums"
        before.append(Hs[0] * wm[0])
    for k in range(W):
        upload(e, wins[k % 8], k)
    e.step(IT, False)
    bad = []
    first = {}
    for k in range(W):
        w = wins[k % 8]
        if k < 8:
            d = fetch(e, k)
            assert e.get_states(window=k)[4] == 0
            bad += check(w, d, levels(w), f"walk G={G} w={k} {w.name}", layers="A")
            first[k] = d
        else:
            d = fetch(e, k, rows=False)
            f = first[k % 8]
            if not (np.array_equal(d["H"], f["H"]) and np.array_equal(d["b"], f["b"]) and d["scalars"][1] == f["scalars"][1]):
                bad.append(f"walk G={G}: window {k} differs from window {k % 8}, the same rows")
    for k in range(W):
        w = wins[k % 8]
        if w.n == N:
            continue
        e.upload_observations(full.xyz, full.uv, full.conf, full.ii, N, window=k)
        got = e.debug("H", window=k)
        if not np.array_equal(got[:w.n], first[k % 8]["H"]):
            bad.append(f"walk G={G}: window {k}: the slots of its own poses changed with the upload")
        tail = got[w.n:] * first[k % 8]["scalars"][1]
        if not any(np.all(np.abs(tail - ref[w.n:]) <= ULP4 * np.abs(ref[w.n:])) for ref in before):
            worst = min(int(np.argmax((np.abs(tail - ref[w.n:]) > ULP4 * np.abs(ref[w.n:])).any((1, 2)))) for ref in before)
            bad.append(f"walk G={G}: window {k} ({w.n} poses): pose slot {w.n + worst} behind its last pose was written")
    e.close()
    assert not bad, "\n".join(bad[:20])


# ------------------------------------------------------------------------------------------------ fp32 Jacobian terms
@pytest.mark.parametrize("G,mode", [(4, 1), (64, 1), (8, 0)])
def test_fp32_jacobian(G, mode):
    """Layer A alone: VBA_DBG_JG hands out the fp32 terms rotated in fp64, so the fp64 sums answer to the fp64 bar.  est and the
    weights carry the bits of the fp64 handle."""
    case = C.clamped(G)
    W = 1 if mode == 1 else 2
    got = {}
    for f32 in (False, True):
        e = engine(case.n, case.m, windows=W, mode=mode, lanes=G, f32=f32)
        for k in range(W):
            upload(e, case, k)
        e.step(IT, False)
        got[f32] = fetch(e, W - 1)
        assert e.get_states(window=W - 1)[4] == 0
        e.close()
    a, b = got[True], got[False]
    assert np.array_equal(a["est"], b["est"]) and np.array_equal(a["w"], b["w"])
    assert not np.array_equal(a["Jg"], b["Jg"]) and rel_err(a["Jg"], b["Jg"]) < 2.0 ** -20
    bad = check(case, a, levels(case), f"fp32 G={G} mode={mode} {case.name}", layers="A")
    bad += check(case, b, levels(case), f"fp64 G={G} mode={mode} {case.name}")
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ bit-exact invariants
@pytest.mark.parametrize("mode", [1, 0])
def test_rows_do_not_depend_on_lanes(mode):
    case = C.clamped(8)
    ref = None
    for G in LANES:
        e = engine(case.n, case.m, windows=1 if mode == 1 else 2, mode=mode, lanes=G)
        for k in range(e.windows):
            upload(e, case, k)
        e.step(IT, False)
        d = fetch(e, e.windows - 1)
        e.close()
        if ref is None:
            ref = d
        assert np.array_equal(d["est"], ref["est"]) and np.array_equal(d["w"], ref["w"]), G
        assert np.array_equal(d["scalars"][:3], ref["scalars"][:3]), G
        assert np.all(d["w"][case.conf == 0] == 0.0)
        empty = case.counts == 0
        assert np.all(d["H"][empty] == 0.0) and np.all(d["b"][empty] == 0.0)
        zero = case.extras["only_zero"]
        assert np.all(d["H"][zero] == 0.0) and np.all(d["b"][zero] == 0.0), "a pose of zero-confidence rows only"


# ------------------------------------------------------------------------------------------------ the whole call
_ORACLE_CHAIN = {}


def oracle_chain(case):
    key = (case.name, case.n, case.m)
    if key not in _ORACLE_CHAIN:
        chain = []
        st, lam = case.states, 1e-4
        for it, init in random_windows.SCHEDULE:
            dbg = {}
            out, lam_out, hess, ntr = O.ba_iteration(it, st, *case.oracle_args(), lam, initialize=init, debug=dbg)
            assert dbg["trials"][-1]["residual"] < dbg["init_residual"]
            chain.append(dict(it=it, init=init, st_in=st, lam_in=lam, out=out, lam=lam_out, hess=hess, ntr=ntr,
                              residual=dbg["trials"][-1]["residual"]))
            st, lam = out, lam_out
        _ORACLE_CHAIN[key] = chain
    return _ORACLE_CHAIN[key]


@pytest.mark.parametrize("mode", [1, 0])
def test_whole_call(mode):
    """clamped(8) through random_windows.SCHEDULE on a default handle, every call from the oracle's state: the bars of
    test_randomised_windows_vs_oracle (test_gpu_parity.py)."""
    from state_metrics import assert_states
    from test_gpu_parity import _attitude_bar
    case = C.clamped(8)
    e = engine(case.n, case.m, mode=mode)
    upload(e, case, states=False)
    args = case.oracle_args()
    for c in oracle_chain(case):
        e.set_states(c["st_in"], c["lam_in"])
        e.step(c["it"], c["init"])
        out, lam, hess, ntr, flags = e.get_states()
        assert flags == 0 and ntr == c["ntr"] and lam == c["lam"], (c["it"], ntr, c["ntr"], lam, c["lam"])
        assert rel_err(out, c["out"]) < 1e-6, c["it"]
        att = _attitude_bar(out, c["out"], 1e-6, lambda sc, solver: O.ba_iteration(c["it"], c["st_in"] * sc, *args, c["lam_in"],
                                                                                    initialize=c["init"], solver=solver)[0])
        err = assert_states(out, c["out"], 1e-6, 1e-6, att, ("clamped(8)", mode, c["it"]))
        assert rel_err(hess, c["hess"]) < 1e-8
        res = e.debug("scalars")[3]
        print(f"FIGURES whole call mode={mode} it={c['it']}: pos {err[0]:.2e} vel {err[1]:.2e} att {err[2]:.2e} rad, trial residual rel "
              f"{rel_err(res, c['residual']):.2e}")
        assert rel_err(res, c["residual"]) < 1e-9, c["it"]
    e.close()
