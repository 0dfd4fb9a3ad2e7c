"""Data snooping on the CPU: the combine rule of vinsat_amd/csrc/vba_snoop_pick.h, compiled for the host, against NumPy's first
arg-max; the selection rule of tests/snoop_oracle.py on a golden window; and the planted-outlier window of
tests/test_gpu_snoop.py through the oracle alone -- the conditions that GPU test relies on are asserted here, where they can be
chosen (tests/snoop_windows.py holds the values)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import rel_oracle as R
import snoop_oracle as S
import snoop_windows as SW
from conftest import ROOT, golden_inputs, load_golden
from oracle import ba_oracle as O

SRC = os.path.join(ROOT, "tests", "hostcheck", "hostcheck_snoop.cpp")
LIB = os.path.join(ROOT, "tests", "hostcheck", "libhostcheck_snoop.so")
P = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def hc():
    hdr = os.path.join(ROOT, "vinsat_amd", "csrc", "vba_snoop_pick.h")
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(f) for f in (SRC, hdr)):
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", LIB, SRC])
    lib = ctypes.CDLL(LIB)
    lib.hc_snoop_fold.argtypes = (ctypes.c_int64, P)
    lib.hc_snoop_butterfly.argtypes = (ctypes.c_int64, P, ctypes.POINTER(ctypes.c_int))
    return lib


def _first_argmax(v):
    """The first position of the largest non-NaN value, or None."""
    ok = ~np.isnan(v)
    if not ok.any():
        return None
    return int(np.nonzero(ok & (v == v[ok].max()))[0][0])


def _sequences():
    rng = np.random.default_rng(15)
    seqs = []
    for _ in range(400):                                        # random, with NaN holes
        v = rng.normal(size=int(rng.integers(1, 70)))
        v[rng.random(v.size) < 0.2] = np.nan
        seqs.append(v)
    for _ in range(400):                                        # tied: few distinct values
        seqs.append(rng.integers(0, 3, int(rng.integers(1, 70))).astype(np.float64))
    for _ in range(100):                                        # tied, with NaN and infinities
        v = rng.choice([np.nan, 1.0, 2.0, np.inf, -np.inf], int(rng.integers(1, 70)))
        seqs.append(v)
    for k in (1, 2, 15, 16, 17, 33, 64):
        seqs += [np.full(k, np.nan), np.full(k, 3.5), np.arange(k, dtype=np.float64), -np.arange(k, dtype=np.float64)]
    seqs += [np.array([2.0]), np.array([np.nan]), np.array([0.0, -0.0]), np.array([-0.0, 0.0])]
    return seqs


def test_combine_rule_against_numpys_first_argmax(hc):
    """The fold in sequence and the fold in the device's shape (16 lanes, strided rows, butterfly over 1, 2, 4, 8) give the first
    position of the maximum; NaN never wins; all-NaN gives no winner; every lane of the butterfly ends with the same winner."""
    none = hc.hc_snoop_no_pos()
    for v in _sequences():
        v = np.ascontiguousarray(v)
        want = _first_argmax(v)
        want = none if want is None else want
        agree = ctypes.c_int(0)
        assert hc.hc_snoop_fold(v.size, v.ctypes.data_as(P)) == want, v
        assert hc.hc_snoop_butterfly(v.size, v.ctypes.data_as(P), ctypes.byref(agree)) == want, v
        assert agree.value == 1, v


def _golden(name):
    g = load_golden(name)
    inp = golden_inputs(g)
    st, lam = g["states_out_19"][0], float(g["lamda_out"][-1])
    d = {}
    O.ba_iteration(19, st, inp["cumrot"], inp["uv"], inp["xyz"], inp["ii"], inp["time_idx"], inp["K"], inp["conf"], lam,
                   initialize=False, debug=d)
    return R.reliability(d, inp["ii"])["wtest"], d["w"], inp["ii"], d["bands"].shape[0]


def test_selection_rule_on_a_golden_window():
    wt, w, ii, n = _golden("c2")
    rows = np.bincount(ii, minlength=n)
    crit = float(np.percentile(wt, 90))
    none, per = S.select(wt, w, ii, n, np.inf, 0, 6)
    assert not none.any() and not per.any()
    for min_rows in (6, int(rows.max()) - 2):
        m0, p0 = S.select(wt, w, ii, n, crit, 0, min_rows)
        m1, p1 = S.select(wt, w, ii, n, crit, 1, min_rows)
        assert m0.any() and (m1 | m0).sum() == m1.sum()                     # mode 1 rejects what mode 0 rejects, and more
        assert m1.sum() > m0.sum() or min_rows > 6
        assert np.bincount(ii[m0], minlength=n).max() <= 1 and np.array_equal(np.bincount(ii[m0], minlength=n), p0)
        for m in (m0, m1):
            left = np.bincount(ii[~m & (w != 0)], minlength=n)
            assert (left[np.bincount(ii[m], minlength=n) > 0] >= min_rows).all()
        # the one row of mode 0 is the pose's first largest candidate
        for i in np.nonzero(p0)[0]:
            k = np.nonzero(ii == i)[0]
            assert np.nonzero(m0)[0][ii[m0] == i][0] == k[np.argmax(wt[k])]
    # a pose that cannot spare a row keeps it; a barred window rejects nothing; NaN and weight-zero rows are no candidates
    assert not S.select(wt, w, ii, n, crit, 0, int(rows.max()))[0].any()
    assert not S.select(wt, w, ii, n, crit, 1, 6, barred=True)[0].any()
    top = int(np.argmax(wt))
    wt2, w2 = wt.copy(), w.copy()
    wt2[top] = np.nan
    assert not S.select(wt2, w, ii, n, crit, 1, 6)[0][top]
    w2[top] = 0.0
    assert not S.select(wt, w2, ii, n, crit, 1, 6)[0][top]
    # the report of close calls: a critical value on a row's wtest, and a tie of the two best
    assert ii[top] in S.ambiguous(wt, w, ii, n, float(wt[top]), 0, 6)
    k = np.nonzero(ii == ii[top])[0]
    wt3 = wt.copy()
    wt3[k[k != top][0]] = wt[top]
    assert ii[top] in S.ambiguous(wt3, w, ii, n, crit, 0, 6)
    assert S.margin_of(wt) == 100.0 * 1e-8 * wt.max()


def test_planted_window_through_the_oracle_alone():
    """What tests/test_gpu_snoop.py relies on.  Measured here (C2, 100 of 5000 detections moved by 300 px, seed 5; crit 6.0 in
    wtest's units, mode 0, min_rows 6, 4 calls per round): rounds reject 67, 26, 6, 1, 0 rows; all 100 planted rows and no other;
    no ambiguous pose (margins 1.7e-4 .. 2.7e-6); mean position error 0.210 km without, 0.092 km with
    snooping."""
    _, _, win, idx = SW.planted()
    res = SW.oracle_loop()
    counts = [int(r["mask"].sum()) for r in res["rounds"]]
    print(f"rounds reject {counts}; margins {[float('%.2g' % r['margin']) for r in res['rounds']]}; planted {idx.size}, found "
          f"{int(res['total'][idx].sum())}, false {int(res['total'].sum() - res['total'][idx].sum())}; mean position error "
          f"{res['err_before']:.4g} -> {res['err_after']:.4g} km")
    assert all(r["ambiguous"] == [] for r in res["rounds"])                 # the cap is zero
    assert res["total"][idx].all()
    assert counts[-1] == 0 and len(counts) <= SW.ROUNDS                     # the loop ends by itself within ROUNDS
