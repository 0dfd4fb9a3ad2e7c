"""The NumPy restatement of the reliability query (tests/rel_oracle.py) at the final states of the golden C1 / C2 windows
(states_out_19, the last lamda_out, iter 19): the identities the definitions imply, the absence of degenerate rows on these
windows, and the spread of the dense references among themselves, which the bars of tests/test_gpu_reliability.py rest on."""
import numpy as np
import pytest

import rel_oracle as R
from conftest import golden_inputs, load_golden
from oracle import ba_oracle as O


def _final(name):
    g = load_golden(name)
    inp = golden_inputs(g)
    st, lam = g["states_out_19"][0], float(g["lamda_out"][-1])
    d = {}
    O.ba_iteration(19, st, inp["cumrot"], inp["uv"], inp["xyz"], inp["ii"], inp["time_idx"], inp["K"], inp["conf"], lam,
                   initialize=False, debug=d)
    return d, inp["ii"], lam


@pytest.mark.parametrize("name", ["c1", "c2"])
def test_trace_identity_and_no_degenerate_row(name):
    """sum_k leverage[k] == sum_i tr(S_i H_i) (H_i = sum_k w_k J_k^T J_k of the pose's rows) to 1e-10 relative; every eigenvalue of
    P_k in (0, 1), every weight positive, every wtest finite: these windows hold no degenerate row."""
    d, ii, lam = _final(name)
    for lam32 in (0.0, float(np.float32(lam))):
        ref = R.reliability(d, ii, lam32)
        tr = float(np.einsum("iab,iba->", ref["S"], d["H"]))
        err = abs(ref["leverage"].sum() - tr) / abs(tr)
        ev = np.linalg.eigvalsh(ref["P"])
        print(f"{name} lam32={lam32:g}: trace identity {err:.2e}; leverage {ref['leverage'].min():.3g} .. {ref['leverage'].max():.3g}; "
              f"eig(P) {ev.min():.3g} .. {ev.max():.3g}; min w {d['w'].min():.3g}; wtest median {np.median(ref['wtest']):.3g} "
              f"max {ref['wtest'].max():.3g}")
        assert err < 1e-10
        assert ev.min() > 0.0 and ev.max() < 1.0
        assert d["w"].min() > 0.0
        assert np.isfinite(ref["wtest"]).all() and np.isfinite(ref["leverage"]).all()
        assert (ref["leverage"] > 0).all() and (ref["leverage"] < 2).all()
        # summary: sums, maxima and counts of the rows
        assert np.allclose(ref["pose_stats"][:, 0].sum(), ref["leverage"].sum(), rtol=1e-13)
        assert ref["pose_stats"][:, 1].max() == ref["wtest"].max()
        assert ref["pose_stats"][:, 2].sum() == ii.size


@pytest.mark.parametrize("name", ["c1", "c2"])
def test_reference_spread_lu_against_cholesky(name):
    """What the 1e-8 bar of the GPU tests rests on: the values from the LU inverse against those from the Cholesky inverse of the
    same system, per row, normalised by the window's largest value.  Measured: leverage 1.1e-10 (c1) / 5.4e-12 (c2), wtest 1.2e-11 /
    1.6e-13.  The bar must hold three times the spread."""
    d, ii, lam = _final(name)
    for lam32 in (0.0, float(np.float32(lam))):
        a, b = R.reliability(d, ii, lam32, method="inv"), R.reliability(d, ii, lam32, method="chol")
        sl, st = R.row_rel_err(a["leverage"], b["leverage"]), R.row_rel_err(a["wtest"], b["wtest"])
        print(f"{name} lam32={lam32:g}: LU vs Cholesky spread: leverage {sl:.2e}, wtest {st:.2e}")
        assert 3.0 * sl < 1e-8 and 3.0 * st < 1e-8


def test_degenerate_rows_are_flagged_in_the_value():
    """A row of weight zero gives 0, 0; a row whose I - P is not positive definite gives NaN."""
    d, ii, lam = _final("c1")
    d = dict(d)
    w = d["w"].copy()
    w[3] = 0.0
    d["w"] = w
    ref = R.reliability(d, ii)
    assert ref["leverage"][3] == 0.0 and ref["wtest"][3] == 0.0
    assert ref["pose_stats"][ii[3], 2] == np.count_nonzero(ii == ii[3]) - 1
    w = d["w"].copy()
    w[5] *= 1e3         # (not a weight the library produces: P_k beyond the unit ball)
    d["w"] = w
    ref = R.reliability(d, ii)
    assert np.isnan(ref["wtest"][5]) and np.isfinite(ref["leverage"][5])
