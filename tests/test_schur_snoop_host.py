"""Free-landmark data snooping (``vba_schur_snoop``) on the CPU: the NumPy rule of tests/schur_snoop_oracle.py on hand-made vectors
that hit every clause; the rule of vinsat_amd/csrc/vba_schur_snoop_pick.h compiled for the host, in the device's shape, against
the NumPy rule on random small groups; the same under the sanitizers as a stand-alone program; and the planted window of
tests/schur_snoop_cases.py through the oracle alone -- the conditions tests/test_gpu_schur_snoop.py relies on are asserted here,
where they can be chosen.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import schur_snoop_cases as SC
import schur_snoop_oracle as SO
from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "hostcheck", "hostcheck_schur_snoop.cpp")
LIB = os.path.join(ROOT, "tests", "hostcheck", "libhostcheck_schur_snoop.so")
NAN = float("nan")


# ------------------------------------------------------------------------------------------------ the rule on hand-made vectors
def _window(tracks, n):
    """Rows from ``{landmark: [poses]}`` in (landmark, pose) order."""
    pr, lr = [], []
    for l, poses in sorted(tracks.items()):
        for i in sorted(poses):
            pr.append(i)
            lr.append(l)
    return np.array(pr), np.array(lr)


def _run(pr, lr, wt, lmwt, n, L, crit=2.0, scaled=False, s0sq=1.0, info=0, w=None, min_rows=0, min_track=3):
    w = np.full(len(pr), 0.95) if w is None else np.asarray(w, dtype=float)
    return SO.select(np.asarray(wt, dtype=float), np.asarray(lmwt, dtype=float), s0sq, info, w, pr, lr, n, L, crit, scaled, min_rows, min_track)


def test_row_against_row_tie_goes_to_the_smaller_sorted_row():
    pr, lr = _window({0: [0, 1, 2]}, 3)
    r = _run(pr, lr, [5.0, 5.0, 3.0], [0.0], 3, 1)
    assert np.array_equal(r["rows"], [True, False, False]) and r["counts"] == (1, 0, 0) and r["margin"] == 0.0
    # ... inside a pose: two landmarks propose rows with equal tests to pose 0; the row of the smaller landmark goes
    pr, lr = _window({0: [0, 1], 1: [0, 2]}, 3)
    r = _run(pr, lr, [4.0, 1.0, 4.0, 1.0], [0.0, 0.0], 3, 2)
    assert np.array_equal(r["rows"], [True, False, False, False])
    # the caller's row order does not matter: the same rows in reverse
    r = _run(pr[::-1], lr[::-1], [1.0, 4.0, 1.0, 4.0], [0.0, 0.0], 3, 2)
    assert np.array_equal(r["rows"], [False, False, False, True])


def test_row_beats_the_prior_on_a_tie_and_the_larger_test_wins_otherwise():
    pr, lr = _window({0: [0, 1, 2]}, 3)
    r = _run(pr, lr, [5.0, 1.0, 1.0], [5.0], 3, 1)
    assert r["rows"][0] and not r["marked"].any() and r["counts"] == (1, 0, 0)
    r = _run(pr, lr, [5.0, 1.0, 1.0], [5.5], 3, 1)
    assert r["marked"][0] and r["landmarks"][0] and r["via"].all() and not r["rows"].any() and r["counts"] == (0, 1, 3)
    r = _run(pr, lr, [5.0, 1.0, 1.0], [4.5], 3, 1)
    assert r["rows"][0] and not r["landmarks"].any()


def test_nan_never_wins():
    pr, lr = _window({0: [0, 1, 2]}, 3)
    r = _run(pr, lr, [NAN, 3.0, 1.0], [NAN], 3, 1)
    assert np.array_equal(r["rows"], [False, True, False]) and not r["marked"].any()
    r = _run(pr, lr, [NAN, NAN, NAN], [NAN], 3, 1)
    assert r["counts"] == (0, 0, 0)
    r = _run(pr, lr, [np.inf, 3.0, 1.0], [np.inf], 3, 1)             # an infinite test is no candidate either
    assert np.array_equal(r["rows"], [False, True, False]) and not r["marked"].any()


def test_zero_weight_rows_are_no_candidates_and_do_not_count():
    pr, lr = _window({0: [0, 1, 2]}, 3)
    r = _run(pr, lr, [9.0, 3.0, 1.0], [0.0], 3, 1, w=[0.0, 0.95, 0.95])
    assert np.array_equal(r["rows"], [False, True, False])
    r = _run(pr, lr, [9.0, 3.0, 1.0], [7.0], 3, 1, w=[0.0, 0.95, 0.95])     # cntl = 2 < min_track: the prior is no candidate
    assert not r["marked"].any() and r["rows"][1]


def test_track_shorter_than_min_track_keeps_its_catalogue_entry():
    pr, lr = _window({0: [0, 1], 1: [0, 1, 2]}, 3)
    r = _run(pr, lr, [0.0] * 5, [9.0, 9.0], 3, 2)
    assert np.array_equal(r["marked"], [False, True]) and np.array_equal(r["landmarks"], [False, True])
    r = _run(pr, lr, [0.0] * 5, [9.0, 9.0], 3, 2, min_track=2)
    assert r["landmarks"].all() and r["counts"] == (0, 2, 5)
    r = _run(pr, lr, [0.0] * 5, [9.0, 9.0], 3, 2, min_track=4)
    assert r["counts"] == (0, 0, 0)


def test_short_pose_cancels_a_marked_landmark_and_nothing_cascades():
    # pose 0 has 3 rows (landmarks 0, 1, 2); landmark 0 is marked; with min_rows = 3 pose 0 would be left with 2: short
    pr, lr = _window({0: [0, 1, 2], 1: [0, 1, 2], 2: [0, 1, 2], 3: [1, 2, 3]}, 4)
    lmwt = [9.0, 0.0, 0.0, 0.0]
    r = _run(pr, lr, [0.0] * 12, lmwt, 4, 4, min_rows=3)
    assert r["marked"][0] and r["short"][0] and not r["landmarks"].any() and r["counts"] == (0, 0, 0)
    r = _run(pr, lr, [0.0] * 12, lmwt, 4, 4, min_rows=2)
    assert r["landmarks"][0] and not r["short"][:3].any() and r["counts"] == (0, 1, 3)       # (pose 3 has one row: short, not concerned)
    # two marked landmarks, one cancelled by pose 3 (one row, min_rows 1): the other still goes -- poses 1 and 2 stay counted
    # without BOTH (cancelling only raises counts), so they reject no row of their own either
    lmwt = [9.0, 0.0, 0.0, 9.0]
    wt = [0.0] * 12
    wt[4] = 8.0                                                     # row (landmark 1, pose 1) is proposed to pose 1
    r = _run(pr, lr, wt, lmwt, 4, 4, min_rows=1)
    assert r["marked"][[0, 3]].all() and r["short"][3] and np.array_equal(r["landmarks"], [True, False, False, False])
    assert r["rows"][4] and r["counts"] == (1, 1, 3)
    r = _run(pr, lr, wt, lmwt, 4, 4, min_rows=2)                    # pose 1: 4 rows, 2 on marked landmarks, 2 - 1 < 2: keeps its row
    assert not r["rows"].any() and not r["short"][1] and r["landmarks"][0]


def test_pose_exactly_at_min_rows_and_one_above():
    pr, lr = _window({l: [0, 1 + l % 2] for l in range(5)}, 3)      # pose 0 has 5 rows
    wt = np.zeros(10)
    wt[0] = 7.0                                                     # (landmark 0, pose 0)
    for min_rows, goes in ((3, True), (4, True), (5, False), (6, False)):
        r = _run(pr, lr, wt, [0.0] * 5, 3, 5, min_rows=min_rows, min_track=3)
        assert bool(r["rows"][0]) == goes and r["short"][0] == (min_rows == 6), min_rows
    w = np.full(10, 0.95)
    w[2] = 0.0                                                      # a zero-weight row of pose 0 does not count: cnt = 4
    assert not _run(pr, lr, wt, [0.0] * 5, 3, 5, w=w, min_rows=4)["rows"].any()
    assert _run(pr, lr, wt, [0.0] * 5, 3, 5, w=w, min_rows=3)["rows"][0]


def test_scaled_critical_value_nan_fit_and_failed_factorisation():
    pr, lr = _window({0: [0, 1, 2]}, 3)
    wt, lmwt = [5.0, 1.0, 1.0], [0.0]
    r = _run(pr, lr, wt, lmwt, 3, 1, crit=2.0, scaled=True, s0sq=4.0)
    assert r["crit_used"] == 4.0 and r["rows"][0]
    r = _run(pr, lr, wt, lmwt, 3, 1, crit=2.0, scaled=True, s0sq=9.0)
    assert r["crit_used"] == 6.0 and r["counts"] == (0, 0, 0)
    s0sq = 138.6243432972694
    assert _run(pr, lr, wt, lmwt, 3, 1, crit=3.29, scaled=True, s0sq=s0sq)["crit_used"] == 3.29 * np.sqrt(s0sq)
    r = _run(pr, lr, wt, lmwt, 3, 1, crit=2.0, scaled=True, s0sq=NAN)
    assert np.isnan(r["crit_used"]) and r["counts"] == (0, 0, 0) and not r["marked"].any()
    r = _run(pr, lr, wt, lmwt, 3, 1, crit=2.0, scaled=False, info=595)
    assert r["crit_used"] == 2.0 and r["counts"] == (0, 0, 0)
    r = _run(pr, lr, wt, lmwt, 3, 1, crit=2.0, scaled=True, s0sq=1.0, info=595)
    assert np.isnan(r["crit_used"]) and r["counts"] == (0, 0, 0)
    assert _run(pr, lr, wt, lmwt, 3, 1, crit=np.inf)["counts"] == (0, 0, 0)


# ------------------------------------------------------------------------------------------------ the header on the host
@pytest.fixture(scope="module")
def hc():
    hdrs = [os.path.join(ROOT, "vinsat_amd", "csrc", f) for f in ("vba_schur_snoop_pick.h", "vba_snoop_pick.h")]
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(f) for f in [SRC] + hdrs):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-o", LIB, SRC])
    return ctypes.CDLL(LIB)


def _random_group(rng, tied):
    n, L = int(rng.integers(1, 21)), int(rng.integers(1, 31))
    tracks = {}
    for l in range(L):
        t = int(rng.integers(0, min(n, 7) + 1))
        tracks[l] = list(rng.choice(n, t, replace=False))
    pr, lr = _window(tracks, n)
    m = pr.size
    if m == 0:
        return None
    if tied:
        wt, lmwt = rng.integers(0, 5, m).astype(float), rng.integers(0, 5, L).astype(float)
    else:
        wt, lmwt = np.abs(rng.normal(0, 2.0, m)), np.abs(rng.normal(0, 2.0, L))
    wt[rng.random(m) < 0.05] = NAN
    lmwt[rng.random(L) < 0.05] = NAN
    w = np.where(rng.random(m) < 0.1, 0.0, 0.95)
    return n, L, pr, lr, wt, lmwt, w


def test_host_build_of_the_rule_agrees_with_numpy_on_random_small_groups(hc):
    """4 000 groups, ties forced (integer tests) in half of them, NaN tests and zero weights sprinkled in, every kind of critical
    value; the butterfly's 16 lanes agree in every pose."""
    from vinsat_amd.schur import build_structure
    rng = np.random.default_rng(31)
    pi, pd, pb = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_ubyte)
    done = rejected = 0
    for rep in range(4000):
        g = _random_group(rng, tied=rep % 2 == 0)
        if g is None:
            continue
        n, L, pr, lr, wt, lmwt, w = g
        perm = rng.permutation(pr.size)                             # the caller's order is any order
        pr, lr, wt, w = pr[perm], lr[perm], wt[perm], w[perm]
        order, s = build_structure(pr, lr, n, L)
        kind = rep % 5
        crit, scaled, s0sq, info = ((2.0, 0, 1.0, 0), (1.0, 1, 4.0, 0), (1.0, 1, NAN, 0), (1.0, 1, 4.0, 595), (0.0, 0, 1.0, 0))[kind]
        min_rows, min_track = int(rng.integers(0, 8)), int(rng.integers(0, 5))
        ref = SO.select(wt, lmwt, s0sq, info, w, pr, lr, n, L, crit, bool(scaled), min_rows, min_track)
        ws, wts = np.ascontiguousarray(w[order]), np.ascontiguousarray(wt[order])
        own, via, rej, used = np.zeros(pr.size, np.uint8), np.zeros(pr.size, np.uint8), np.zeros(L, np.uint8), ctypes.c_double()
        agree = hc.hc_schur_snoop(n, L, int(pr.size), *[s[k].ctypes.data_as(pi) for k in ("lm_ptr", "row_pose", "row_lm", "pose_ptr", "pose_rows")],
                                  ws.ctypes.data_as(pd), wts.ctypes.data_as(pd), lmwt.ctypes.data_as(pd), ctypes.c_double(s0sq), info,
                                  ctypes.c_double(crit), scaled, min_rows, min_track, own.ctypes.data_as(pb), rej.ctypes.data_as(pb),
                                  via.ctypes.data_as(pb), ctypes.byref(used))
        assert agree == 1
        assert np.array_equal(own != 0, ref["rows"][order]) and np.array_equal(via != 0, ref["via"][order]) and np.array_equal(rej != 0, ref["landmarks"]), rep
        assert used.value == ref["crit_used"] or (np.isnan(used.value) and np.isnan(ref["crit_used"]))
        done += 1
        rejected += sum(ref["counts"])
    assert done > 3500 and rejected > 3000


def test_rule_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """A stand-alone program with its own main (CPU only); any ASan / UBSan finding aborts it with a non-zero code."""
    src = os.path.join(ROOT, "tests", "hostcheck", "sanitize_schur_snoop_main.cpp")
    exe = str(tmp_path / "sanitize_schur_snoop_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, src])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "sanitize_schur_snoop_main ok" in p.stdout and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr


def test_ctypes_prototypes_and_header_agree():
    import re
    from vinsat_amd import _lib
    sig = _lib.SIGNATURES
    assert sig["vba_schur_snoop"][1][1:6] == [ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    with open(os.path.join(ROOT, "include", "vinsat_ba.h")) as f:
        hdr = f.read()
    assert re.search(r"int vba_schur_snoop\(vba_schur_handle h, double lamda, double crit, int scaled, int min_rows, int min_track, int\* counts[^;]*"
                     r"double\* crit_used[^;]*int\* info\);", hdr)
    assert re.search(r"int vba_schur_rejected\(vba_schur_handle h, unsigned char\* row_mask[^;]*unsigned char\* lm_mask[^;]*int\* totals[^;]*\);", hdr)
    assert re.search(r"int vba_schur_snoop_restore\(vba_schur_handle h\);", hdr) and re.search(r"int vba_schur_last_snoop_ms\(vba_schur_handle h, float\* ms\);", hdr)
    from vinsat_amd.schur import SchurBA
    assert all(hasattr(SchurBA, k) for k in ("snoop", "rejected", "restore_rejected", "last_snoop_ms"))


# ------------------------------------------------------------------------------------------------ the planted window
def test_planted_window_through_the_oracle_alone():
    """What tests/test_gpu_schur_snoop.py relies on.  Measured here ("43": 5 501 rows, 100 detections moved by 40 px on 100 distinct
    tracks of >= 4, 5 catalogue entries moved by 10 sigma, seed 7; crit 5.5 scaled, min_rows 6, min_track 3, query at lamda 1e-3):
    rounds reject (rows, landmarks, rows through landmarks) (39, 0, 0), (31, 0, 0), (13, 0, 0), (11, 0, 0), (6, 0, 0), (0, 5, 63),
    (0, 0, 0) with crit_used 28.7, 22.6, 16.4, 12.9, 8.87, 5.59, 5.54; every planted row and every displaced entry, nothing else;
    smallest margin of a decided comparison 4.9e-3 (round 3) against a bar of 5.4e-8: 9e4 bars; mean pose position error 2.101 km
    after the first solve, 1.367 km at the end."""
    d, res = SC.planted(), SC.oracle_loop()
    for k, r in enumerate(res["rounds"]):
        print(f"FIGURES schur snoop planted round {k}: counts {r['counts']} crit_used {r['crit_used']:.4g} s0sq {r['s0sq']:.4g} "
              f"margin {r['margin']:.3g} bar {r['bar']:.3g}")
    print(f"FIGURES schur snoop planted: mean position error {res['err_before']:.4g} -> {res['err_after']:.4g} km")
    assert len(res["rounds"]) <= SC.SNOOP["rounds"] and res["rounds"][-1]["counts"] == (0, 0, 0)
    assert tuple(r["counts"] for r in res["rounds"]) == SC.EXPECTED_ROUNDS
    assert np.array_equal(np.nonzero(res["rows"])[0], d["planted_rows"])                # every planted row, and no other
    assert np.array_equal(np.nonzero(res["landmarks"])[0], d["displaced_lms"])
    for r in res["rounds"]:
        assert r["margin"] >= r["bar"]                              # (the bar already holds the factor 100)
    assert d["planted_rows"].size == SC.N_ROWS and 0.015 < SC.N_ROWS / d["w"].size < 0.025 and SC.N_LANDMARKS / d["X0"].shape[0] > 0.01
