"""CPU side of the free-landmark covariance query (``vba_schur_covariance``): the reference of tests/schur_cov_cases.py against
itself.  No GPU.

Floors (disagreement of the reference's two NumPy routes, relative to the largest entry of the family), as measured:

  case                          lam    pose       pairs      landmark   cond(S)
  12 / 150                      0      4.7e-13    4.7e-13    3.3e-14    4.2e9
  12 / 150                      1e-3   2.3e-13    4.0e-13    2.4e-14    4.2e9
  43 / 450                      0      4.7e-13    4.7e-13    1.2e-14    5.7e9
  43 / 450                      1e-3   4.0e-13    4.0e-13    1.5e-14    5.7e9
  128 / 1300                    1e-3   1.1e-13    1.1e-13    1.5e-14    7.8e9
  129 / 1300                    1e-3   2.2e-13    2.2e-13    1.5e-14    7.5e9
  wide                          1e-3   1.5e-13    3.6e-13    1.9e-14    9.7e9
  pose_without_rows             1e-3   2.3e-16    3.6e-16    6.7e-14    7.4e12
  more_landmarks_than_rows      0      1.1e-12    1.1e-12    3.8e-14    9.8e9
  more_landmarks_than_rows      1e-3   4.3e-13    4.3e-13    1.9e-14    9.7e9
  more_poses_than_landmarks     1e-3   3.5e-11    3.5e-11    1.8e-12    1.2e11
  behind_the_camera             1e4    1.9e-9     1.9e-9     2.0e-9     7.4e5     (the clamp case: printed, not bounded)

(they move by a few tens of per cent with the BLAS and its thread count).  A bar of the GPU tests is
``max(100 x floor, 1e-11)``: the floors are held below 1e-10 here so that no bar can silently grow.
"""
import numpy as np
import pytest

import schur_cov_cases as V


@pytest.mark.parametrize("name,lam", V.CASES)
def test_floor_of_the_reference(name, lam):
    r = V.reference(name, lam)
    print(f"FIGURES floor {name} lam={lam:g} " + " ".join(f"{k}={r.floor[k]:.2e}" for k in V.FAMILIES) + f" cond(S)={r.condS:.2e}")
    assert all(np.isfinite(r.floor[k]) for k in V.FAMILIES)
    if name != V.CLAMP:
        assert max(r.floor.values()) < 1e-10
    # pairs holds the diagonal blocks too
    dg = r.blk_i == r.blk_j
    assert np.array_equal(r.blk_i[dg], np.arange(r.pose.shape[0])) and np.array_equal(r.pairs[dg], r.pose)


@pytest.mark.parametrize("name,lam", [("43", 0.0), ("43", 1e-3), ("more_landmarks_than_rows", 0.0), ("12", 0.0)])
def test_orderings_of_the_reference(name, lam):
    """What freeing the landmarks means: a landmark ends inside its prior and outside its conditional, a pose outside its
    frozen-landmark covariance.  To 1e-9 of the prior variance."""
    r = V.reference(name, lam)
    m = V.definiteness(r.pose, r.landmark, r)
    print(f"FIGURES orderings {name} lam={lam:g} " + " ".join(f"{k}={v:.2e}" for k, v in m.items()))
    assert m["below_prior"] >= -1e-9                # (holds at lam > 0 as well: damping only shrinks the covariance)
    assert m["above_conditional"] >= -1e-9
    assert m["pose_above_frozen"] >= -1e-9


def test_unobserved_landmarks_of_the_reference_keep_their_prior():
    d = V.case("more_landmarks_than_rows")
    for lam in (0.0, 1e-3):
        r = V.reference("more_landmarks_than_rows", lam)
        closed = 1.0 / (1.0 / (d["sigma"] * d["sigma"]) + lam)
        assert np.abs(r.landmark[d["unobserved"]] - closed * np.eye(3)).max() <= 1e-14 * closed


def test_sigma_helpers():
    from vinsat_amd import schur
    r = V.reference("12", 0.0)
    pos, att = schur.pose_sigmas(dict(pose=r.pose, landmark=r.landmark))
    dg = np.diagonal(r.pose, axis1=1, axis2=2)
    assert np.array_equal(pos, np.sqrt(dg[:, :3])) and np.array_equal(att, 2.0 * np.sqrt(dg[:, 3:]))
    assert np.array_equal(schur.pose_sigmas(r.pose)[1], att)
    assert np.array_equal(schur.landmark_sigmas(r.landmark), np.sqrt(np.diagonal(r.landmark, axis1=1, axis2=2)))


def test_ctypes_prototypes_and_header_agree():
    import ctypes
    import os
    import re
    from vinsat_amd import _lib
    sig = _lib.SIGNATURES
    assert sig["vba_schur_covariance"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_double, _lib.PD, _lib.PD, _lib.PD, ctypes.POINTER(ctypes.c_int)])
    assert sig["vba_schur_last_covariance_ms"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)])
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vinsat_ba.h")) as f:
        hdr = f.read()
    assert re.search(r"int vba_schur_covariance\(vba_schur_handle h, double lamda, double\* pose_cov[^;]*double\* pair_cov[^;]*double\* lm_cov[^;]*int\* info\);", hdr)
    assert re.search(r"int vba_schur_last_covariance_ms\(vba_schur_handle h, float\* ms\);", hdr)
    if os.path.exists(_lib.LIB_PATH):               # the built library exports both (it is loaded without a device)
        lib = ctypes.CDLL(_lib.LIB_PATH)
        assert lib.vba_schur_covariance and lib.vba_schur_last_covariance_ms
