"""CPU side of the state-covariance query of a handle with the dynamics factor (``vba_schur_covariance_dyn``,
``SchurBA.state_covariance``): the reference of tests/schur_dyn_cov_cases.py against itself, the NumPy restatement of the device's
gather and the mistakes it must be able to tell, the tile list of the selected product, and the host build of
vinsat_amd/csrc/vba_schur_dyn_cov.h under the sanitizers as a stand-alone program.  No GPU.

Floors (disagreement of the reference's two NumPy routes, every entry scaled by the reference sigmas of its row and column), at
``schur_dyn_cases.SIGMA_DYN`` = 1e4, as measured:

  case        lam     state     edges     pairs     landmark  cond(S9)
  12 / 150    0       3.1e-10   2.8e-10   3.1e-10   1.1e-12   7e9
  12 / 150    1e-3    7.9e-10   7.6e-10   7.9e-10   6.9e-13   7e9
  29 / 300    0       7.3e-11   7.4e-11   7.3e-11   4.4e-13   3e9
  29 / 300    1e-3    3.6e-11   3.6e-11   3.6e-11   1.7e-13   3e9
  43 / 450    1e-3    1.5e-11   1.5e-11   1.5e-11   8.6e-14   9e12
  86 / 900    0       1.3e-11   1.3e-11   1.3e-11   4.1e-14   2e9
  86 / 900    1e-3    1.2e-11   1.2e-11   1.2e-11   2.9e-14   2e9

(they move by a few tens of per cent with the BLAS and its thread count).  A bar of the GPU tests is ``max(100 x floor, 1e-11)``:
the floors are held below 1e-8 here so that no bar can silently grow (at sigma_dyn = 1e6 they reach 4.5e-9: the cases stay at
SIGMA_DYN).
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import schur_cases as SC
import schur_dyn_cov_cases as V
import schur_dyn_oracle as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name,lam", V.CASES)
def test_floor_of_the_reference(name, lam):
    r = V.reference(name, lam)
    print(f"FIGURES floor {name} lam={lam:g} " + " ".join(f"{k}={r.floor[k]:.2e}" for k in V.FAMILIES) + f" cond(S9)={r.condS:.2e}")
    assert all(np.isfinite(r.floor[k]) for k in V.FAMILIES)
    assert max(r.floor.values()) < 1e-8
    # pairs holds the diagonal blocks, and they are the pose parts of the state blocks
    dg = r.blk_i == r.blk_j
    assert np.array_equal(r.blk_i[dg], np.arange(r.n)) and np.array_equal(r.pairs[dg], r.state[:, :6, :6])


def test_cases_reach_the_edges_their_names_say():
    tiles = lambda N: (N + V.TILE - 1) // V.TILE
    panels = lambda N: (N + 255) // 256
    shape = {name: V.case(name)["states0"].shape[0] for name in ("12", "29", "43", "86")}
    assert shape == {"12": 12, "29": 29, "43": 43, "86": 86}
    assert (tiles(108), panels(108), 72 // 64, 72 % 64) == (2, 1, 1, 8)
    assert (tiles(261), panels(261), 174 // 64) == (5, 2, 2) and 174 % 64 != 0
    assert (tiles(774), panels(774), 516 // 64, 516 % 64) == (13, 4, 8, 4)
    assert set(np.diff(V.case("12")["time_idx"])) == {1} and set(np.diff(V.case("29")["time_idx"])) == {1, 5, 64}
    assert not np.any(V.case("43")["pose_of_row"] == 20)


def _stored(r):
    """S9^-1 in the lower triangle, the transposed factor above it: what an upper-triangle read would meet."""
    return np.tril(r.Sinv) + np.triu(r.Lc.T, 1)


@pytest.mark.parametrize("name", ("12", "29", "86"))
def test_restatement_of_the_gather(name):
    """The index map u, the lower-triangle read and the edge orientation: the gather from the stored triangle alone gives the
    blocks the oracle's own unknown order cuts out of the full symmetric matrix, bit for bit."""
    r = V.reference(name, 1e-3)
    n = r.n
    state, edges = V.gather(_stored(r), n)
    sym = np.tril(r.Sinv) + np.tril(r.Sinv, -1).T
    want = V.families(sym, r.landmark, n, r.blk_i, r.blk_j)
    assert np.array_equal(state, want["state"]) and np.array_equal(edges, want["edges"])
    assert np.array_equal(state, np.swapaxes(state, 1, 2))
    idx = D.unknown_index(n)
    assert np.array_equal(V.unknown(n, np.arange(n)[:, None], np.arange(9)[None, :]), idx)
    # rows of pose i, columns of pose i + 1: the velocity of pose i against the position of pose i + 1 sits at [6:, :3]
    i = n // 2
    assert np.array_equal(edges[i][6:, :3], sym[np.ix_(idx[i, 6:], idx[i + 1, :3])])
    assert np.array_equal(edges[i][:3, 6:], sym[np.ix_(idx[i, :3], idx[i + 1, 6:])])
    # and they are what the reference holds, to its floor
    fig = V.scaled(dict(state=state, edges=edges, pairs=want["pairs"], landmark=r.landmark), r)
    assert fig["state"] <= 2 * r.floor["state"] + 1e-15 and fig["edges"] <= 2 * r.floor["edges"] + 1e-15


@pytest.mark.parametrize("fault", V.FAULTS)
def test_planted_faults_are_past_the_bars(fault):
    """Each mistake the gather could make moves the state or the edge family by at least ten bars on 29 / 300."""
    r = V.reference("29", 1e-3)
    state, edges = V.gather(_stored(r), r.n, fault=fault)
    fig = V.scaled(dict(state=state, edges=edges, pairs=r.pairs, landmark=r.landmark), r)
    bars = {k: fig[k] / V.bar(r, k) for k in ("state", "edges")}
    print(f"FAULT {fault}: " + " ".join(f"{k}={fig[k]:.1e} ({bars[k]:.1e} bars)" for k in bars))
    assert max(bars.values()) >= 10.0, bars


@pytest.mark.parametrize("name", ("12", "29", "86"))
def test_tile_list_covers_what_the_gathers_read_and_nothing_else(name):
    d = V.case(name)
    n = d["states0"].shape[0]
    s = V.structure(d)
    rows, cols = V.read_entries(n, s["blk_i"].astype(np.int64), s["blk_j"].astype(np.int64))
    assert np.all(rows >= cols) and rows.max() < 9 * n
    tiles = V.listed_tiles(n, s["blk_i"].astype(np.int64), s["blk_j"].astype(np.int64))
    nbu = (9 * n + V.TILE - 1) // V.TILE
    assert all(0 <= J <= I < nbu for I, J in tiles)
    print(f"TILES {name}: {len(tiles)} of {nbu * (nbu + 1) // 2}")
    b = 6 * n // V.TILE                               # the tile the pose / velocity boundary lies in
    assert (6 * n) % V.TILE != 0 and (b, b) in tiles
    if name == "86":
        assert len(tiles) < 0.6 * (nbu * (nbu + 1) // 2)  # velocity tiles far from the pose band: nearly half of the 91 tiles are skipped
        assert (nbu - 1, 0) not in tiles and (nbu - 1, (6 * (n - 1)) // V.TILE) in tiles


def test_failure_case_is_singular_for_the_reference_too():
    """43 / 450 at lamda = 0: pose 20 has no rows and there is no attitude factor, so its attitude rows of S9 are exactly zero.  The
    unpivoted Cholesky stops at row 6 * 20 + 3, and the dense inverse of the reference route refuses the matrix."""
    B9, Cm, E9, S9 = V.failure_system()
    assert not S9[123:126].any() and not S9[:, 123:126].any()
    row, _ = SC.first_bad_pivot(S9)
    assert row == 6 * 20 + 3 == 123
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.inv(np.block([[B9, E9], [E9.T, Cm]]))


def test_state_sigmas():
    from vinsat_amd import schur
    r = V.reference("12", 0.0)
    pos, att, vel = schur.state_sigmas(dict(state=r.state))
    dg = np.diagonal(r.state, axis1=1, axis2=2)
    assert np.array_equal(pos, np.sqrt(dg[:, :3])) and np.array_equal(att, 2.0 * np.sqrt(dg[:, 3:6])) and np.array_equal(vel, np.sqrt(dg[:, 6:]))
    assert np.array_equal(schur.state_sigmas(r.state)[2], vel)
    assert np.array_equal(schur.pose_sigmas(r.state[:, :6, :6])[1], att)


def test_ctypes_prototypes_and_header_agree():
    from vinsat_amd import _lib
    sig = _lib.SIGNATURES
    assert sig["vba_schur_covariance_dyn"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_double, _lib.PD, _lib.PD, _lib.PD, _lib.PD,
                                                              ctypes.POINTER(ctypes.c_int)])
    assert sig["vba_schur_last_covariance_dyn_ms"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)])
    with open(os.path.join(ROOT, "include", "vinsat_ba.h")) as f:
        hdr = f.read()
    assert re.search(r"int vba_schur_covariance_dyn\(vba_schur_handle h, double lamda, double\* state_cov[^;]*double\* edge_cov[^;]*"
                     r"double\* pair_cov[^;]*double\* lm_cov[^;]*int\* info\);", hdr)
    assert re.search(r"int vba_schur_last_covariance_dyn_ms\(vba_schur_handle h, float\* ms\);", hdr)
    if os.path.exists(_lib.LIB_PATH):               # the built library exports both (it is loaded without a device)
        lib = ctypes.CDLL(_lib.LIB_PATH)
        assert lib.vba_schur_covariance_dyn and lib.vba_schur_last_covariance_dyn_ms


def test_host_build_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """vba_schur_dyn_cov.h compiled for the host: the gathers' index map and the tile-list builder for n = 2, 12, 29, 86 with
    blocks that straddle tile edges.  Every entry read lies in a listed tile at or below the diagonal, every listed tile is read."""
    src = os.path.join(ROOT, "tests", "hostcheck", "sanitize_schur_dyn_cov_main.cpp")
    exe = str(tmp_path / "sanitize_schur_dyn_cov_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, src])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "sanitize_schur_dyn_cov_main ok" in p.stdout and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
